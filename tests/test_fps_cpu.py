"""CPU checks of tests/fps_ref.py, the float32 statement of vision3d's two furthest-point sampling loops that the GPU tests lean on: it has to
reproduce every list the reference's own programs produced (tests/golden/fps.npz), and the library has to refuse what it documents -- the
refusals come before any launch, so they need no GPU."""
import ctypes
import os

import numpy as np
import pytest

from tests import fps_ref as F
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "fps.npz"))


def test_fixture_names_its_programs_and_margins(gold):
    assert "native_furthest_point_sample" in list(gold["programs"])
    for name, n, _, md, ns in F.SCENES:
        assert gold[name + "/points"].shape == (n, 3) and gold[name + "/points"].dtype == np.float32
        win, stop = gold[name + "/margins"]
        assert win > 1e-5 and stop > 1e-5, (name, win, stop)
    # the three stop rules, and with both rules given each of the two is the one that stops in some scene
    both = {name: (len(gold[name + "/indices"]), ns) for name, _, _, md, ns in F.SCENES if md is not None and ns is not None}
    assert any(k == ns for k, ns in both.values())
    assert 1 < both[F.STOPPED_BY_MIN_DISTANCE_WITH_BOTH_RULES][0] < both[F.STOPPED_BY_MIN_DISTANCE_WITH_BOTH_RULES][1]
    assert any(md is None for _, _, _, md, ns in F.SCENES) and any(ns is None for _, _, _, md, ns in F.SCENES)


@pytest.mark.parametrize("scene", [s[0] for s in F.SCENES])
def test_statement_reproduces_the_reference(gold, scene):
    _, n, _, md, ns = next(s for s in F.SCENES if s[0] == scene)
    idx, dist, status = F.nodes(gold[scene + "/points"], md, ns)
    assert status == 0
    assert np.array_equal(idx, gold[scene + "/indices"])
    assert np.array_equal(dist.view(np.uint32), gold[scene + "/distances"].view(np.uint32))
    assert dist[0] == 0 and np.all(np.diff(dist[1:]) <= 0)
    if ns is not None:
        assert len(idx) <= ns
    if md is not None:
        assert np.all(dist[1:] >= np.float32(md))


@pytest.mark.parametrize("scene,M", [("n64", 64), ("n65", 7), ("n1025", 33)])
def test_batch_statement_is_the_node_statement_on_squared_distances(gold, scene, M):
    pts = gold[scene + "/points"]
    want = F.nodes(pts, None, M, squared=True)[0]
    assert np.array_equal(F.batch(pts[None], M)[0], want)


def test_batch_statement_repeats_the_lowest_index_beyond_n():
    pts = np.arange(15, dtype=np.float32).reshape(5, 3) ** 2
    got = F.batch(pts[None], 9)[0]
    assert sorted(got[:5]) == [0, 1, 2, 3, 4] and np.all(got[5:] == 0)


def test_statement_rules():
    lattice = np.stack(np.meshgrid(np.arange(4.0), np.arange(4.0), np.arange(1.0), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    idx, dist, _ = F.nodes(lattice, None, 3)
    assert list(idx) == [0, 15, 3]                           # (0, 3) and (3, 0) tie at distance 3: the lowest index wins
    pts = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [np.inf, 0, 0]], np.float32)
    idx, _, st = F.nodes(pts, None, 4)
    assert list(idx) == [0, 2] and st == F.ST_NONFINITE      # non-finite points are never taken; the cloud is used up
    assert F.nodes(pts[1:], None, 2)[2] == F.ST_NONFINITE | F.ST_START and len(F.nodes(pts[1:], None, 2)[0]) == 0
    assert len(F.nodes(np.zeros((5, 3), np.float32), 0.1, None)[0]) == 1       # identical points: every distance is 0
    assert F.nodes(lattice, 0.5, None, sample_cap=4)[2] == F.ST_CAP
    assert F.nodes(lattice, 0.5, 4, sample_cap=4)[2] == 0
    for md, ns in ((None, None), (0.0, None), (-1.0, None)):
        with pytest.raises(ValueError):
            F.nodes(lattice, md, ns)


def test_library_refuses_before_any_launch():
    from diffreg_hip import lib
    raw = lib.raw()
    assert raw.dr_fps_onchip_capacity() >= 9000
    cap = raw.dr_fps_onchip_capacity()
    assert raw.dr_fps_workspace_bytes(1, 100, 100) == 0 and raw.dr_fps_workspace_bytes(2, cap + 1, cap + 1) >= 4 * (cap + 1)
    fake = ctypes.c_void_p(4096)                             # never dereferenced: every call below is refused on the host
    EINVAL, ENOSUP, EWORKSPACE = -1, -3, -4
    nodes = lambda P=1, n=10, mx=10, pts=fake, off=fake, md=0.1, ns=-1, cap_=4, idx=fake, cnt=fake, st=fake, ws=None, wsb=0: \
        raw.dr_fps_nodes_f32(P, n, mx, pts, off, md, ns, cap_, idx, None, None, cnt, st, ws, wsb, None)
    assert nodes(P=0) == 0
    for kw in (dict(P=-1), dict(n=-1), dict(mx=11), dict(pts=None), dict(off=None), dict(idx=None), dict(cnt=None), dict(st=None), dict(cap_=0),
               dict(md=0.0), dict(md=-1.0), dict(md=float("nan"))):
        assert nodes(**kw) == EINVAL, kw
    assert nodes(P=70000) == ENOSUP
    assert nodes(n=cap + 1, mx=cap + 1) == EWORKSPACE
    assert nodes(n=cap + 1, mx=cap + 1, ws=fake, wsb=16) == EWORKSPACE
    assert nodes(n=cap + 1, mx=cap + 1, ws=ctypes.c_void_p(4100), wsb=1 << 20) == EINVAL
    batch = lambda B=1, N=8, M=4, pts=fake, idx=fake, ws=None, wsb=0: raw.dr_fps_batch_f32(B, N, M, pts, idx, ws, wsb, None)
    assert batch(B=0) == 0 and batch(M=0) == 0
    for kw in (dict(B=-1), dict(N=-1), dict(M=-1), dict(N=0), dict(pts=None), dict(idx=None)):
        assert batch(**kw) == EINVAL, kw
    assert batch(B=60000, N=60000) == ENOSUP
    assert batch(N=cap + 1) == EWORKSPACE


def test_python_refusals():
    import torch
    from diffreg_hip import nonrigid
    pts = torch.zeros(4, 3)
    for kw in (dict(), dict(min_distance=0.0), dict(num_samples=0), dict(min_distance=0.1, sample_cap=0), dict(num_samples=2, lengths=[3])):
        with pytest.raises(ValueError):
            nonrigid.fps_nodes(pts, **kw)
    with pytest.raises(TypeError):
        nonrigid.fps_nodes(pts.double(), num_samples=2)
    for call in (lambda: nonrigid.fps_nodes(pts, num_samples=2), lambda: nonrigid.fps_nodes(pts, 0.1, lengths=[1, 3]),
                 lambda: nonrigid.furthest_point_sample_nodes(pts, 0.1), lambda: nonrigid.furthest_point_sample(pts[None], 2),
                 lambda: nonrigid.NonRigidRegistration(node_sampler="fps").sample_nodes_fps([pts])):
        with pytest.raises(TypeError, match="on the GPU"):   # a host tensor's pointer is never handed to a kernel
            call()
    with pytest.raises(ValueError):
        nonrigid.NonRigidRegistration(node_sampler="random")
    assert nonrigid.NonRigidRegistration().node_sampler == "grid"
