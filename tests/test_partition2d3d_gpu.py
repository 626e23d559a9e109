"""GPU: the device entries of csrc/partition2d3d.hip through diffreg_hip.partition2d3d against the fixture minted by running the reference (scenes a-c of
tests/golden/partition2d3d.npz) and against the float64 restatement at a size the fixture does not hold (scene d), under the decided / undecided rules of
tests/partition2d3d_ref.py."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import partition2d3d_ref as R
from tests.conftest import ROOT
from tests.helpers import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(ROOT, "tests", "golden", "partition2d3d.npz")
PART_KEYS = ("point_to_node", "node_sizes", "node_masks", "node_knn_indices", "node_knn_masks")
CORR_KEYS = ("img_corr_indices", "pcd_corr_indices", "img_corr_overlaps", "pcd_corr_overlaps", "pcd_centers", "img_centers", "img_centers_da", "coarse_match_gt")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def P():
    from diffreg_hip import partition2d3d
    return partition2d3d


def dev(sc):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in sc.items()}


def run_partition(P, d, **kw):
    return dict(zip(PART_KEYS, P.point_to_node_partition(d["pcd_points"], d["nodes"], d["limit"], return_count=True, gather_points=True, **kw)))


def run_patchify(P, d, stride=None, Hc=None, Wc=None):
    return P.patchify(d["img_points"], d["img_points_da"], d["img_pixels"], d["img_masks"], d["img_masks_da"], d["H"], d["W"], Hc or d["Hc"], Wc or d["Wc"],
                      stride=stride or d["stride"])


def run_chain(P, d, **kw):
    """EXP/model.py:403-495 on the device entries"""
    part = run_partition(P, d)
    patches = run_patchify(P, d)
    args = R.node_corr_inputs(d, part, DEV, patches=patches)
    out = dict(zip(CORR_KEYS, P.get_2d3d_node_correspondences(*R.reference_args(args), **kw)))
    return part, patches, args, out


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_partition_vs_golden(golden, P, name):
    sc = R.make_scene(name)
    assert np.array_equal(R.input_checksum(sc), golden[name + "_input_checksum"])
    got = run_partition(P, dev(sc))
    assert got["point_to_node"].dtype == torch.int64 and got["node_knn_indices"].dtype == torch.int64 and got["node_knn_masks"].dtype == torch.bool
    ref = R.partition(sc["pcd_points"], sc["nodes"], sc["limit"], want_gaps=True)
    st = R.assert_partition_matches(got, ref, sc["pcd_points"].shape[0], sc["limit"], name)
    print("scene %s: undecided points %d, nodes touched %d, positions compared as sets %d" % ((name,) + st))
    # and against the reference's own arrays: identical wherever the restatement decides (both were just held to it); the shapes are the reference's
    assert tuple(got["node_knn_indices"].shape) == golden[name + "_node_knn_indices"].shape
    und = ref["gap2"].numpy() < R.GAP2
    assert np.array_equal(got["point_to_node"].cpu().numpy()[~und], golden[name + "_point_to_node"][~und])


def test_patchify_vs_golden(golden, P):
    sc = R.make_scene("a")
    p = run_patchify(P, dev(sc))
    assert np.array_equal(p[3].cpu().numpy(), golden["a_patch_knn_indices"]) and p[3].dtype == torch.int64
    for t, k in zip(p[4:], ("knn_masks", "knn_masks_da", "masks", "masks_da")):
        assert t.dtype == torch.bool and np.array_equal(t.cpu().numpy(), golden["a_patch_" + k])
    q = R.patchify(sc["img_points"], sc["img_points_da"], sc["img_pixels"], sc["img_masks"], sc["img_masks_da"], sc["H"], sc["W"], sc["Hc"], sc["Wc"], sc["stride"])
    for a, b in zip(p[:3], q[:3]):
        assert torch.equal(a.cpu(), b)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_node_correspondences_vs_golden(golden, P, name):
    sc = R.make_scene(name)
    part, _, args, out = run_chain(P, dev(sc))
    # decidedness is judged on the restatement fed with the DEVICE's partition (its patches differ from the reference's at undecided points only)
    ref = R.ref_node_corr({k: v.cpu() for k, v in args.items()}, want_undecided=True)
    n, und = R.assert_overlaps_match(out, ref, sc["nodes"].shape[0], name)
    print("scene %s: %d candidates, %d pairs, %d undecided; the reference lists %d" % (name, ref["cand_i"].shape[0], n, und, golden[name + "_img_corr_indices"].shape[0]))
    assert out["img_corr_indices"].dtype == torch.int64 and out["img_corr_overlaps"].dtype == torch.float32 and out["coarse_match_gt"].dtype == torch.int64
    R.assert_mutual_matches(out["coarse_match_gt"], out["pcd_centers"].cpu(), out["img_centers"].cpu(), R.R_MUTUAL, name)
    # the reference's list itself: on the reference's own partition (the stored arrays) the device must reproduce the stored pairs wherever decided
    gpart = {k: torch.from_numpy(golden["%s_%s" % (name, k)].astype(np.int64) if golden["%s_%s" % (name, k)].dtype == np.int32 else golden["%s_%s" % (name, k)])
             for k in PART_KEYS}
    args_g = R.node_corr_inputs(sc, gpart)
    ref_g = R.ref_node_corr(args_g, want_undecided=True)
    out_g = dict(zip(CORR_KEYS, P.get_2d3d_node_correspondences(*[a.to(DEV) if torch.is_tensor(a) else a for a in R.reference_args(args_g)])))
    R.assert_overlaps_match(out_g, ref_g, sc["nodes"].shape[0], name + " (reference's partition)")
    N = sc["nodes"].shape[0]
    ck = ref_g["cand_i"].numpy() * N + ref_g["cand_j"].numpy()
    und_of = lambda i, j: ref_g["undecided"].numpy()[np.searchsorted(ck, i.astype(np.int64) * N + j)]
    gi, gj = golden[name + "_img_corr_indices"], golden[name + "_pcd_corr_indices"]
    di, dj = out_g["img_corr_indices"].cpu().numpy(), out_g["pcd_corr_indices"].cpu().numpy()
    kg, kd = ~und_of(gi, gj), ~und_of(di, dj)
    assert np.array_equal(gi[kg], di[kd]) and np.array_equal(gj[kg], dj[kd])
    for k in ("img_corr_overlaps", "pcd_corr_overlaps"):
        assert np.array_equal(golden["%s_%s" % (name, k)][kg].view(np.uint32), out_g[k].cpu().numpy()[kd].view(np.uint32)), k
    for k in ("pcd_centers", "img_centers", "img_centers_da"):
        assert np.abs(out_g[k].cpu().numpy() - golden["%s_%s" % (name, k)]).max() <= R.TOL_CENTER, k
    R.assert_mutual_matches(golden[name + "_coarse_match_gt"], out_g["pcd_centers"].cpu(), out_g["img_centers"].cpu(), R.R_MUTUAL, name)


def test_second_size_vs_restatement(P):
    """scene d: other Nf, Nc, limit; patchify at two levels with stride 1 (Ki = 64 and 256)"""
    sc = R.make_scene("d")
    d = dev(sc)
    got = run_partition(P, d)
    ref = R.partition(sc["pcd_points"], sc["nodes"], sc["limit"], want_gaps=True)
    R.assert_partition_matches(got, ref, sc["pcd_points"].shape[0], sc["limit"], "d")
    for Hc, Wc in ((sc["Hc"], sc["Wc"]), (sc["Hc"] // 2, sc["Wc"] // 2)):
        p = run_patchify(P, d, stride=1, Hc=Hc, Wc=Wc)
        q = R.patchify(sc["img_points"], sc["img_points_da"], sc["img_pixels"], sc["img_masks"], sc["img_masks_da"], sc["H"], sc["W"], Hc, Wc, 1)
        assert p[0].shape[1] == (sc["H"] // Hc) * (sc["W"] // Wc)
        for a, b in zip(p, q):
            assert torch.equal(a.cpu(), b)
        args = R.node_corr_inputs(d, got, DEV, patches=p)
        out = dict(zip(CORR_KEYS, P.get_2d3d_node_correspondences(*R.reference_args(args))))
        refc = R.ref_node_corr({k: v.cpu() for k, v in args.items()}, want_undecided=True)
        n, und = R.assert_overlaps_match(out, refc, sc["nodes"].shape[0], "d %dx%d" % (Hc, Wc))
        assert n > 0
        R.assert_mutual_matches(out["coarse_match_gt"], out["pcd_centers"].cpu(), out["img_centers"].cpu(), R.R_MUTUAL, "d")


def test_width_given_makes_no_host_read(P):
    """width = point_limit: the whole call is captured into a graph (a host read of the device would fail the capture); the replay equals the eager call"""
    sc = R.make_scene("b")
    d = dev(sc)
    eager = run_partition(P, d, width=d["limit"])
    assert eager["node_knn_indices"].shape[1] == d["limit"]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = run_partition(P, d, width=d["limit"])
    g.replay()
    torch.cuda.synchronize()
    for k in PART_KEYS:
        assert torch.equal(cap[k], eager[k]), k
    with pytest.raises(ValueError):
        run_partition(P, d, width=d["limit"] + 1)
    with pytest.raises(RuntimeError):        # DR_ENOSUP: point_limit beyond 128
        P.point_to_node_partition(d["pcd_points"], d["nodes"], 129, return_count=True)


def test_candidate_capacity_overflow_is_an_error(P):
    sc = R.make_scene("c")
    d = dev(sc)
    _, _, args, out = run_chain(P, d)
    with pytest.raises(RuntimeError, match="capacity"):
        P.get_2d3d_node_correspondences(*R.reference_args(args), capacity=10)
    raw = P.node_correspondences_raw(args["img_masks"], args["img_kp"], args["img_kp_da"], args["img_kx"], args["img_km"], args["img_km_da"], args["pcd_masks"],
                                     args["pcd_kp"], args["pcd_kx"], args["pcd_km"], args["transform"], R.R2D, R.R3D, capacity=10)
    n, kept, found = raw["counts"].tolist()
    assert kept == 10 and found > 10 and n <= 10
    # room for exactly the candidates: the full result
    full = P.get_2d3d_node_correspondences(*R.reference_args(args), capacity=found)
    assert torch.equal(full[0], out["img_corr_indices"]) and torch.equal(full[2], out["img_corr_overlaps"])
    with pytest.raises(RuntimeError, match="capacity"):
        P.get_correspondences(d["nodes"], d["pcd_points"], None, 0.5, capacity=5)


def test_radius_pairs_and_mutual_nn_vs_float64(P):
    sc = R.make_scene("c")
    d = dev(sc)
    src = sc["nodes"]
    cam = sc["pcd_points"] @ sc["transform"][:3, :3].T + sc["transform"][:3, 3]          # targets in the camera frame: the transform takes the sources there
    ident = torch.eye(4)
    for T, tgt, r in ((sc["transform"], cam, 0.06), (sc["transform"].numpy(), cam, 0.9), (None, sc["pcd_points"], 0.2), (ident, sc["pcd_points"], 0.2)):
        got = P.get_correspondences(P.to_o3d_pcd(d["nodes"]), P.to_o3d_pcd(tgt.to(DEV)), T, r)
        assert got.dtype == torch.int64 and got.dim() == 2 and got.shape[1] == 2 and got.is_cuda
        Tt = None if T is None else torch.as_tensor(T)
        inside, near = R.assert_radius_pairs_match(got, src, tgt, Tt, r, "r=%g" % r)
        print("radius %g: %d pairs inside, %d within the margin" % (r, inside, near))
        assert inside > 0
    assert P.get_correspondences(d["nodes"], d["pcd_points"], None, 1e-9).shape == (0, 2)          # empty result
    assert P.get_correspondences(d["nodes"][:0], d["pcd_points"], None, 1.0).shape == (0, 2)
    a, b = d["nodes"], d["pcd_points"][::7].contiguous()
    for r in (0.06, 0.3, 1e-9):
        got = P.multual_nn_correspondence(a, b, search_radius=r)
        assert got.dtype == torch.int64 and got.shape[0] == 2
        R.assert_mutual_matches(got, a.cpu(), b.cpu(), r, "r=%g" % r)
    assert P.multual_nn_correspondence(a, b, search_radius=1e-9).shape == (2, 0)
    assert P.multual_nn_correspondence(a[:0], b, search_radius=1.0).shape == (2, 0)


def test_two_runs_are_bit_identical(P):
    d = dev(R.make_scene("a"))
    runs = []
    for _ in range(2):
        part, patches, _, out = run_chain(P, d)
        pairs = P.get_correspondences(d["nodes"], out["img_centers"], d["transform"], 0.1)
        runs.append(list(part.values()) + list(patches) + list(out.values()) + [pairs])
    for a, b in zip(*runs):          # byte for byte (floats by their bit patterns)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_nothing_written_outside_the_counts(P):
    """the lists live between guard bands and are pre-filled: rows beyond the written count keep the fill"""
    sc = R.make_scene("c")
    d = dev(sc)
    _, _, args, ref_out = run_chain(P, d)
    cap = 4096
    bufs = [guarded((cap,), dt, DEV, fill=fill) for dt, fill in ((torch.int64, -7), (torch.int64, -7), (torch.float32, -7.0), (torch.float32, -7.0))]
    raw = P.node_correspondences_raw(args["img_masks"], args["img_kp"], args["img_kp_da"], args["img_kx"], args["img_km"], args["img_km_da"], args["pcd_masks"],
                                     args["pcd_kp"], args["pcd_kx"], args["pcd_km"], args["transform"], R.R2D, R.R3D, capacity=cap, out=tuple(b[0] for b in bufs))
    n = int(raw["counts"][0])
    assert n == ref_out["img_corr_indices"].shape[0] and 0 < n < cap
    for (t, chk), k in zip(bufs, CORR_KEYS[:4]):
        chk()
        assert torch.equal(t[:n], ref_out[k]) and bool((t[n:] == -7).all()), k
    pb = [guarded((cap,), torch.int64, DEV, fill=-7) for _ in range(2)]
    i, j, counts = P.radius_pairs_raw(d["nodes"], d["pcd_points"], None, 0.06, capacity=cap, out=(pb[0][0], pb[1][0]))
    m = int(counts[0])
    assert 0 < m < cap and int(counts[1]) == m
    for t, chk in pb:
        chk()
        assert bool((t[m:] == -7).all()) and bool((t[:m] >= 0).all())


def _stand_in_module():
    """a module whose globals hold the names EXP/model.py imports, and a model class defined in it whose forward calls them inline"""
    mod = types.ModuleType("partition_overlay_stand_in")
    src = '''
import torch
def point_to_node_partition(*a, **k): return "original partition"
def patchify(*a, **k): return "original patchify"
def get_2d3d_node_correspondences(*a, **k): return "original correspondences"
def get_correspondences(*a, **k): return "original search"
def to_o3d_pcd(x): return "original wrap"
class Stub(torch.nn.Module):
    def forward(self, x): return x
class Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.denoising_transformer, self.denoising_coarse_matching, self.transformer, self.coarse_matching = Stub(), Stub(), Stub(), Stub()
    def get_warped_from_noising_matching3D3D(self, *a): return a
    def names(self):
        return point_to_node_partition, patchify, get_2d3d_node_correspondences, get_correspondences, to_o3d_pcd
'''
    exec(compile(src, mod.__name__, "exec"), mod.__dict__)
    sys.modules[mod.__name__] = mod
    mod.Model.__module__ = mod.__name__
    return mod


def test_overlay_partition_flag(P):
    from diffreg_hip.overlay2d3d import accelerate
    mod = _stand_in_module()
    try:
        model = mod.Model()
        before = model.names()
        ov = accelerate(model)                                       # flag off: no global is touched
        assert model.names() == before
        ov.remove()
        ov = accelerate(model, partition=True)                       # eval: the three names of model.py:403-495
        now = model.names()
        assert now[:3] == (P.point_to_node_partition, P.patchify, P.get_2d3d_node_correspondences) and now[3:] == before[3:]
        d = dev(R.make_scene("c"))
        out = now[0](d["pcd_points"], d["nodes"], d["limit"], gather_points=True, return_count=True)      # the call as model.py:403-409 writes it
        assert len(out) == 5 and out[3].shape[0] == d["nodes"].shape[0]
        ov.remove()
        assert model.names() == before
        ov = accelerate(model, training=True, partition=True)        # training: the GT search as well
        assert model.names() == (P.point_to_node_partition, P.patchify, P.get_2d3d_node_correspondences, P.get_correspondences, P.to_o3d_pcd)
        ov.remove()
        assert model.names() == before and not hasattr(model, "_dr_overlay")
    finally:
        sys.modules.pop(mod.__name__, None)
