"""Every entry whose workspace has one carve (csrc/carve.h), run on a workspace of exactly the queried size between guard bands.  Needs a GPU.

Each case calls its entry through lib.raw() on identical inputs:
  1. with a workspace that is a slice of exactly the queried size, 4096 bytes into a byte tensor filled with 0xA5 (4096 guard bytes each side);
  2. with a workspace of twice the queried size;
  3. offered one byte less than the queried size.
Calls 1 and 2 return DR_OK, every output tensor is bit-equal between them and both guard bands are still 0xA5.  Call 3 returns
DR_EWORKSPACE and launches nothing: every output keeps its prefill, except the scalars the entry clears BEFORE it looks at the workspace (the
documented order of its early returns) -- those are zero.  dr_match_recall_f32 takes no workspace size, so it has no call 3.

Shapes: the smallest that put every array of the layout on the far side of a 256-byte boundary of the one before it (an extent of 65 4-byte
elements, a padded length of 128, two clouds, a second workgroup of hypotheses: iters = 257), recorded in each case."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DR_OK, DR_EWORKSPACE = 0, -4
GUARD = 4096
FILL = {torch.float32: 7.25, torch.float64: 7.25, torch.int32: -7, torch.int64: -7, torch.uint8: 0x5A}


@pytest.fixture(scope="module", autouse=True)
def _init():
    from diffreg_hip import lib
    lib.ensure_init()


def out(shape, dtype, fill=None):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), FILL[dtype] if fill is None else fill, dtype=dtype, device=DEV)


def bits(t):
    return t.contiguous().view(torch.uint8)


def three_calls(wsb, run, cleared=(), short_call=True):
    """run(ws_ptr, ws_bytes) -> (rc, dict of fresh, prefilled output tensors the entry was given)"""
    wsb = int(wsb)
    assert wsb > 0
    buf = torch.full((GUARD + wsb + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    rc1, o1 = run(ctypes.c_void_p(buf.data_ptr() + GUARD), wsb)
    big = torch.full((2 * wsb,), 0xA5, dtype=torch.uint8, device=DEV)
    rc2, o2 = run(ctypes.c_void_p(big.data_ptr()), 2 * wsb)
    torch.cuda.synchronize()
    assert rc1 == DR_OK and rc2 == DR_OK, (rc1, rc2)
    assert bool((buf[:GUARD] == 0xA5).all()), "the entry wrote in front of its workspace"
    assert bool((buf[GUARD + wsb:] == 0xA5).all()), "the entry wrote behind its workspace"
    assert sorted(o1) == sorted(o2)
    for k in o1:
        assert torch.equal(bits(o1[k]), bits(o2[k])), "output %s differs between the exact-size and the double-size workspace" % k
    if not short_call:
        return o1
    rc3, o3 = run(ctypes.c_void_p(buf.data_ptr() + GUARD), wsb - 1)
    torch.cuda.synchronize()
    assert rc3 == DR_EWORKSPACE, rc3
    for k, t in o3.items():
        want = torch.zeros_like(t) if k in cleared else out(tuple(t.shape), t.dtype, fill=0 if k == "hist" else None)
        assert torch.equal(bits(t), bits(want)), "a call refused with DR_EWORKSPACE changed " + k
    return o1


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * scale).to(DEV).contiguous()


def i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


def test_point_to_node_partition():
    from diffreg_hip import lib
    raw, p = lib.raw(), lib.ptr
    Nf, Nc, K = 65, 3, 4                      # padded to 128: keys 1024 bytes, values 512
    pts, nodes = rnd(Nf, 3, seed=1), rnd(Nc, 3, seed=2)

    def run(ws, wsb):
        o = dict(p2n=out(Nf, torch.int64), sizes=out(Nc, torch.int64), masks=out(Nc, torch.uint8), knn=out((Nc, K), torch.int64),
                 knn_masks=out((Nc, K), torch.uint8), mx=out(1, torch.int32))
        rc = raw.dr_point_to_node_partition_f32(Nf, Nc, K, p(pts), p(nodes), p(o["p2n"]), p(o["sizes"]), p(o["masks"]), p(o["knn"]), p(o["knn_masks"]),
                                                p(o["mx"]), ws, wsb, lib.stream_of(pts))
        return rc, o
    o = three_calls(raw.dr_point_to_node_partition_workspace_bytes(Nf), run)
    assert int(o["sizes"].sum()) == Nf


def test_unique_pairs():
    from diffreg_hip import lib
    raw, p = lib.raw(), lib.ptr
    n = 65
    g = torch.Generator().manual_seed(3)
    a, b = torch.randint(0, 6, (n,), generator=g).to(DEV), torch.randint(0, 6, (n,), generator=g).to(DEV)

    def run(ws, wsb):
        o = dict(keys=out(n, torch.int64), count=out(1, torch.int32))
        return raw.dr_unique_pairs_i64(n, p(a), p(b), 8, p(o["keys"]), p(o["count"]), ws, wsb, lib.stream_of(a)), o
    o = three_calls(raw.dr_unique_pairs_workspace_bytes(n), run)
    assert int(o["count"]) == torch.unique(a * 8 + b).numel()


def test_grid_subsample():
    from diffreg_hip import lib
    raw, p = lib.raw(), lib.ptr
    n, nb = 65, 2                             # CloudInfo rows 72 bytes, keys 1024, values 512, one scan block
    pts, lengths = rnd(n, 3, seed=4), i32([30, 35])

    def run(ws, wsb):
        o = dict(points=out((n, 3), torch.float32), lengths=out(nb, torch.int32), total=out(1, torch.int32), status=out(1, torch.int32))
        rc = raw.dr_grid_subsample_f32(n, nb, p(pts), p(lengths), 0.3, p(o["points"]), p(o["lengths"]), p(o["total"]), p(o["status"]), ws, wsb,
                                       lib.stream_of(pts))
        return rc, o
    o = three_calls(raw.dr_grid_subsample_workspace_bytes(n, nb), run, cleared=("lengths", "total", "status"))
    assert int(o["status"]) == 0 and 0 < int(o["total"]) <= n and int(o["lengths"].sum()) == int(o["total"])


def ball_inputs():
    nq, ns, nb = 7, 65, 2                     # two CloudInfo tables, keys 1024, values 512, sorted 1040, cell table 4096 bytes
    return nq, ns, nb, rnd(nq, 3, seed=5), rnd(ns, 3, seed=6), i32([3, 4]), i32([30, 35])


def test_radius_neighbors():
    from diffreg_hip import lib
    raw, p = lib.raw(), lib.ptr
    nq, ns, nb, q, s, ql, sl = ball_inputs()
    limit = 8

    def run(ws, wsb):
        o = dict(idx=out((nq, limit), torch.int64), max_count=out(1, torch.int32), status=out(1, torch.int32))
        rc = raw.dr_radius_neighbors_f32(nq, ns, nb, p(q), p(s), p(ql), p(sl), 0.4, limit, p(o["idx"]), p(o["max_count"]), p(o["status"]), ws, wsb,
                                         lib.stream_of(q))
        return rc, o
    o = three_calls(raw.dr_radius_neighbors_workspace_bytes(nq, ns, nb), run, cleared=("max_count", "status"))
    assert int(o["status"]) == 0


def test_radius_count_hist():
    from diffreg_hip import lib
    raw, p = lib.raw(), lib.ptr
    nq, ns, nb, q, s, ql, sl = ball_inputs()
    bins = 80

    def run(ws, wsb):
        o = dict(hist=out(bins, torch.int32, fill=0), counts=out(nq, torch.int32), status=out(1, torch.int32))    # (the caller zeroes the histogram)
        rc = raw.dr_radius_count_hist_f32(nq, ns, nb, p(q), p(s), p(ql), p(sl), 0.4, bins, p(o["hist"]), p(o["counts"]), p(o["status"]), ws, wsb,
                                          lib.stream_of(q))
        return rc, o
    o = three_calls(raw.dr_radius_count_hist_workspace_bytes(nq, ns, nb), run, cleared=("status",))
    assert int(o["status"]) == 0 and int(o["hist"].sum()) == nq


def test_node_correspondences():
    from diffreg_hip import lib
    raw, p = lib.raw(), lib.ptr
    M, N, Ki, Kc, cap = 3, 5, 4, 4, 15        # eight arrays of 240, 12, 12, 20, 60, 60, 60, 60 bytes: each starts a new 256-byte block
    ones = lambda *sh: torch.ones(*sh, dtype=torch.uint8, device=DEV)
    im, ikm, ikmd, pm, pkm = ones(M), ones(M, Ki), ones(M, Ki), ones(N), ones(N, Kc)
    ip, ipd, ix = rnd(M, Ki, 3, seed=7), rnd(M, Ki, 3, seed=8), rnd(M, Ki, 2, seed=9, scale=40.0)
    pp, px = rnd(N, Kc, 3, seed=10), rnd(N, Kc, 2, seed=11, scale=40.0)
    T = torch.eye(4, device=DEV)

    def run(ws, wsb):
        o = dict(ii=out(cap, torch.int64), pi=out(cap, torch.int64), io=out(cap, torch.float32), po=out(cap, torch.float32), counts=out(3, torch.int32),
                 pc=out((N, 3), torch.float32), ic=out((M, 3), torch.float32), icd=out((M, 3), torch.float32))
        rc = raw.dr_node_correspondences_2d3d_f32(M, Ki, N, Kc, p(im), p(ip), p(ipd), p(ix), p(ikm), p(ikmd), p(pm), p(pp), p(px),
                                                  p(pkm), p(T), 30.0, 0.6, cap, p(o["ii"]), p(o["pi"]), p(o["io"]), p(o["po"]), p(o["counts"]),
                                                  p(o["pc"]), p(o["ic"]), p(o["icd"]), ws, wsb, lib.stream_of(ip))
        return rc, o
    o = three_calls(raw.dr_node_correspondences_2d3d_workspace_bytes(M, N, Kc, cap), run)
    n, kept, found = o["counts"].tolist()
    assert 0 <= n <= kept <= cap and kept <= found


def test_mutual_nn_radius():
    from diffreg_hip import lib
    raw, p = lib.raw(), lib.ptr
    ns, nt = 65, 3                            # 260, 260, 12, 12 bytes
    src, tgt = rnd(ns, 3, seed=12), rnd(nt, 3, seed=13)

    def run(ws, wsb):
        o = dict(src=out(ns, torch.int64), tgt=out(ns, torch.int64), count=out(1, torch.int32))
        return raw.dr_mutual_nn_radius_f32(ns, nt, p(src), p(tgt), 0.5, p(o["src"]), p(o["tgt"]), p(o["count"]), ws, wsb, lib.stream_of(src)), o
    o = three_calls(raw.dr_mutual_nn_radius_workspace_bytes(ns, nt), run)
    assert 0 <= int(o["count"]) <= nt


def test_radius_pairs():
    from diffreg_hip import lib
    raw, p = lib.raw(), lib.ptr
    ns, nt = 65, 3                            # moved sources 780 bytes, row counts 260
    cap = ns * nt
    src, tgt = rnd(ns, 3, seed=14), rnd(nt, 3, seed=15)
    T = torch.eye(4, device=DEV)

    def run(ws, wsb):
        o = dict(src=out(cap, torch.int64), tgt=out(cap, torch.int64), counts=out(2, torch.int32))
        rc = raw.dr_radius_pairs_f32(ns, nt, p(src), p(tgt), p(T), 0.5, cap, p(o["src"]), p(o["tgt"]), p(o["counts"]), ws, wsb, lib.stream_of(src))
        return rc, o
    o = three_calls(raw.dr_radius_pairs_workspace_bytes(ns, nt), run)
    assert 0 <= int(o["counts"][0]) <= cap


def test_ransac():
    from diffreg_hip import lib
    raw, p = lib.raw(), lib.ptr
    P, cap, N, iters = 2, 5, 6, 257           # RS_BLOCK + 1: two workgroups per pair; their 64 bytes of bests end inside a 256-byte block
    s = rnd(P, N, 3, seed=16)
    t = (s.roll(1, -1) + 0.25).contiguous()      # a rotation (cyclic axis permutation) and a shift
    matches = torch.zeros(P, cap, 3, dtype=torch.int64)
    for b in range(P):
        for k in range(cap):
            matches[b, k] = torch.tensor([b, k, k])
    matches, count = matches.to(DEV), i32([5, 4])

    def run(ws, wsb):
        o = dict(rot=out((P, 3, 3), torch.float64), trn=out((P, 3), torch.float64), fit=out(P, torch.float64), rmse=out(P, torch.float64),
                 best=out(P, torch.int32))
        rc = raw.dr_ransac_corr_f64(P, cap, N, N, p(matches), p(count), p(s), p(t), 0.05, iters, 5, None, p(o["rot"]), p(o["trn"]), p(o["fit"]),
                                    p(o["rmse"]), p(o["best"]), ws, wsb, lib.stream_of(s))
        return rc, o
    three_calls(raw.dr_ransac_workspace_bytes(P, cap, iters), run)


def test_pnp_ransac():
    from diffreg_hip import lib
    raw, p = lib.raw(), lib.ptr
    n, iters = 5, 257                         # two workgroups: 208 bytes of bests, then the inlier bytes
    X = rnd(n, 3, seed=17)
    X[:, 2] += 1.5
    fx, fy, cx, cy = 500.0, 510.0, 320.0, 240.0
    px = torch.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], dim=1).contiguous()
    K = (ctypes.c_double * 9)(fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0)

    def run(ws, wsb):
        o = dict(T=out((4, 4), torch.float64), n_inlier=out(1, torch.int32), best=out(1, torch.int32))
        rc = raw.dr_pnp_ransac_f64(n, p(X), p(px), 0, K, iters, 8.0, 3, p(o["T"]), p(o["n_inlier"]), p(o["best"]), ws, wsb, lib.stream_of(X))
        return rc, o
    three_calls(raw.dr_pnp_ransac_workspace_bytes(n, iters), run)


def test_mutual_topk():
    from diffreg_hip import lib
    raw, p = lib.raw(), lib.ptr
    B, N, M, k = 3, 9, 9, 2                   # 3 words per element: 36 bytes of bits, then the counts in the next 256-byte block
    cap = B * min(N, M) * k
    score = rnd(B, N, M, seed=18)

    def run(ws, wsb):
        o = dict(idx=out((cap, 3), torch.int64), score=out(cap, torch.float32), total=out(1, torch.int32))
        rc = raw.dr_mutual_topk_select_f32(B, N, M, p(score), k, 1, 0, 0.0, 1, None, None, p(o["idx"]), p(o["score"]), cap, p(o["total"]), ws, wsb,
                                           lib.stream_of(score))
        return rc, o
    o = three_calls(raw.dr_mutual_topk_workspace_bytes(B, N, M), run, cleared=("total",))
    assert 0 <= int(o["total"]) <= cap


def test_procrustes_workspace_form():
    from diffreg_hip import lib
    raw, p = lib.raw(), lib.ptr
    P, N, M = 3, 257, 256                     # N * M > 65536: the chip-wide selection on the workspace; P * 4 = 12 bytes of list lengths
    conf, s, t = rnd(P, N, M, seed=19), rnd(P, N, 3, seed=20), rnd(P, M, 3, seed=21)

    def run(ws, wsb):
        o = dict(R=out((P, 3, 3), torch.float32), t=out((P, 3), torch.float32), Rf=out((P, 3, 3), torch.float32), tf=out((P, 3), torch.float32),
                 cond=out(P, torch.float64), ok=out(P, torch.int32))
        rc = raw.dr_procrustes_f32(P, N, M, p(conf), p(s), p(t), None, None, 0, 0.5, 1e9, p(o["R"]), p(o["t"]), p(o["Rf"]), p(o["tf"]), p(o["cond"]),
                                   p(o["ok"]), None, ws, wsb, lib.stream_of(conf))
        forms.append(int(raw.dr_debug_procrustes_last_form()))
        return rc, o
    forms = []
    three_calls(raw.dr_procrustes_workspace_bytes(P, N, M), run)
    assert forms[0] in (1, 2) and forms[1] in (1, 2), "the workspace form did not run"


def test_match_recall():
    from diffreg_hip import lib
    raw, p = lib.raw(), lib.ptr
    P, N, M, K = 1, 5, 5, 3                   # 32768 bytes of partials, then 25 mark bytes
    gt = torch.zeros(P, N, M)
    gt[0, 0, 0] = gt[0, 1, 2] = gt[0, 3, 3] = gt[0, 4, 1] = 1.0
    gt = gt.to(DEV)
    pred = torch.tensor([[0, 0, 0], [0, 1, 2], [0, 2, 2]], dtype=torch.int64, device=DEV)

    def run(ws, wsb):
        o = dict(rp=out(2, torch.float32))
        return raw.dr_match_recall_f32(P, N, M, p(gt), K, p(pred), p(o["rp"]), ws, lib.stream_of(gt)), o
    o = three_calls(raw.dr_train_workspace_bytes(P, N, M), run, short_call=False)
    assert torch.allclose(o["rp"].cpu(), torch.tensor([0.5, 2.0 / 3.0]))        # (recall 2 of 4, precision 2 of 3)


def test_top1_union_row_block_form():
    from diffreg_hip import lib
    raw, p = lib.raw(), lib.ptr
    P, N, M = 2, 33, 5                        # three row blocks of 16; 264 bytes of row keys (16-byte rounding: 272), 64 of slack
    conf = rnd(P, N, M, seed=22)

    def run(ws, wsb):
        o = dict(matches=out((P, N + M, 3), torch.int64), count=out(P, torch.int32))
        return raw.dr_top1_union_f32(P, N, M, p(conf), p(o["matches"]), p(o["count"]), ws, wsb, lib.stream_of(conf)), o
    o = three_calls(raw.dr_top1_union_workspace_bytes(P, N, M, 4), run)
    assert bool(((o["count"] > 0) & (o["count"] <= N + M)).all())
