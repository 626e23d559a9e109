"""GPU checks of the Gauss-Newton non-rigid ICP entries (csrc/nonrigid_gn.hip) through the C ABI, against the reference's recorded float64
outputs (tests/golden/nonrigid_gn.npz and nonrigid_gn_A.npz: vision3d's own non_rigid_icp_gauss_newton run on the CPU).

The bar is the Adam entries' (tests/nonrigid_ref.ratio <= 1): per tensor, the deviation from the reference's float64 is at most max(one float32
ulp at the tensor's largest magnitude, 4 x the reference's own recorded float32 deviation).  Every comparison prints its ratio before it asserts.
dr_spd_solve_f64 is held to a normwise backward error: at most max(n 2^-52, 4 x numpy.linalg.solve's on the same system)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import nonrigid_gn_ref as G
from tests import nonrigid_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(s, f) for s in G.SCENES for f in G.FORMS]
B = G.BLOCK
WORST = {"ratio": 0.0}


@pytest.fixture(scope="module")
def gold():
    return G.load(GOLDEN)


@pytest.fixture(scope="module")
def nr():
    from diffreg_hip import nonrigid
    return nonrigid


def dev(a):
    a = np.asarray(a)
    return torch.from_numpy(a.astype(np.float32) if a.dtype.kind == "f" else a.astype(np.int64)).to(DEV).contiguous()


def host(t):
    return t.detach().cpu().numpy()


def held(what, got, ref64, dev32=None):
    r = R.ratio(host(got) if isinstance(got, torch.Tensor) else got, ref64, dev32)
    WORST["ratio"] = max(WORST["ratio"], r)
    print("%-52s deviation / bar = %.3f   (largest so far %.3f)" % (what, r, WORST["ratio"]))
    assert r <= 1.0, (what, r)
    return r


def problem_of(nr, inp):
    return nr.Problem(dev(inp["nodes"]), dev(inp["src"]), dev(inp["tgt"]), dev(inp["ai"]), dev(inp["aw"]), dev(inp["edges"]), dev(inp["ew"]))


def call_args(inp, form):
    """the keyword arguments of nicp_gauss_newton / nicp_gn_normal for a form of the fixture"""
    lc, la, lm, has_cw, has_ew = G.FORMS[form]
    return dict(corr_lambda=lc, arap_lambda=la, lm_lambda=lm, corr_weights=dev(inp["cw"]) if has_cw else None, unit_edge_weights=not has_ew)


@pytest.fixture(scope="module")
def runs(nr, gold):
    """the device solver on every scene and form, once: {(scene, form): {n: transforms}}; every call is made twice and must be bit-equal"""
    out = {}
    for s, f in CASES:
        inp = G.scene_inputs(gold, s)
        pb, kw = problem_of(nr, inp), call_args(inp, f)
        out[(s, f)] = {}
        for n in G.ITERS:
            T, status = nr.nicp_gauss_newton(pb, num_iterations=n, **kw)
            T2, status2 = nr.nicp_gauss_newton(pb, num_iterations=n, **kw)
            assert int(status.abs().sum()) == 0 and torch.equal(T, T2) and torch.equal(status, status2)
            out[(s, f)][n] = T
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("scene,form", CASES)
def test_transforms(gold, runs, scene, form):
    key = "%s_%s_" % (scene, form)
    for n in G.ITERS:
        T = host(runs[(scene, form)][n])
        assert np.isfinite(T).all() and np.array_equal(T[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (T.shape[0], 1)))
        held("%s %s transforms after %d" % (scene, form, n), T[:, :3], gold[key + "T%d" % n], gold[key + "T%d_dev32" % n])


@pytest.mark.parametrize("scene,form", CASES)
def test_normal_equations(nr, gold, scene, form):
    """A and b at the identity state and at the reference's state after iteration 1 (rounded to float32, which is what the device can read)"""
    inp = G.scene_inputs(gold, scene)
    pb, kw = problem_of(nr, inp), call_args(inp, form)
    M, key = inp["nodes"].shape[0], "%s_%s_" % (scene, form)
    for it in range(G.RECORD):
        if it == 0:
            rot, trn = np.tile(np.eye(3), (M, 1, 1)), np.zeros((M, 3))
        else:
            T1 = gold[key + "T1"]
            rot, trn = T1[:, :, :3], T1[:, :, 3]
        A, b, status = nr.nicp_gn_normal(pb, dev(rot), dev(trn), **kw)
        A2, b2, _ = nr.nicp_gn_normal(pb, dev(rot), dev(trn), **kw)
        assert int(status.abs().sum()) == 0 and torch.equal(A, A2) and torch.equal(b, b2)
        A, b = host(A[0]), host(b[0])
        assert np.array_equal(A, A.T) or np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max()
        held("%s %s b of iteration %d" % (scene, form, it + 1), b, gold[key + "b%d" % it], gold[key + "b%d_dev32" % it])
        assert (key + "A%d" % it in gold) == G.has_A(scene, form, M)
        if key + "A%d" % it in gold:
            ref = gold[key + "A%d" % it]
            held("%s %s A of iteration %d" % (scene, form, it + 1), A if ref.ndim == 2 else G.tril_pack(A), ref, gold[key + "A%d_dev32" % it])


def test_resume_2_plus_3_is_5(nr, gold, runs):
    for scene, form in (("c", "mod"), ("i", "fn"), ("d", "now")):
        inp = G.scene_inputs(gold, scene)
        pb, kw = problem_of(nr, inp), call_args(inp, form)
        st = nr.new_gn_state(pb)
        T2, _ = nr.nicp_gauss_newton(pb, num_iterations=2, state=st, **kw)
        assert torch.equal(T2, runs[(scene, form)][2])
        T5, _ = nr.nicp_gauss_newton(pb, num_iterations=3, state=st, resume=True, **kw)
        assert torch.equal(T5, runs[(scene, form)][5])
        assert torch.equal(st["rotations"], T5[:, :3, :3]) and torch.equal(st["translations"], T5[:, :3, 3])
        T0, _ = nr.nicp_gauss_newton(pb, num_iterations=0, **kw)
        assert torch.equal(T0, torch.eye(4, device=DEV).expand(T0.shape[0], 4, 4))


def test_python_names_return_the_ragged_form(nr, gold, runs):
    inp = G.scene_inputs(gold, "g")
    a = [dev(inp[k]) for k in ("nodes", "src", "tgt", "ai", "aw", "edges")]
    T = nr.non_rigid_icp_gauss_newton(*a, edge_weights=dev(inp["ew"]))
    assert torch.equal(T, runs[("g", "fn")][5])
    T = nr.non_rigid_icp_gauss_newton(*a)                                        # edge_weights=None
    assert torch.equal(T, runs[("g", "now")][5])
    layer = nr.NonRigidICP()
    assert repr(layer) == "NonRigidICP(corr_lambda=1, arap_lambda=1, lm_lambda=0.01, num_iterations=5)"
    T = layer(*a, corr_weights=dev(inp["cw"]), edge_weights=dev(inp["ew"]))
    assert torch.equal(T, runs[("g", "mod")][5])
    T = nr.non_rigid_icp_gauss_newton(*a, corr_weights=dev(inp["cw"]), edge_weights=dev(inp["ew"]), arap_lambda=0.0, num_iterations=2)
    assert torch.equal(T, runs[("g", "noarap")][2])


@pytest.mark.parametrize("scene", ("c", "i"))
def test_registration_with_gauss_newton(nr, gold, runs, scene):
    """graph -> Gauss-Newton -> warp of the whole cloud, against the reference's apply_deformation of the reference's transforms, as recorded in
    both precisions (the restated apply_deformation must give the recorded float64 warp too)"""
    inp = G.scene_inputs(gold, scene)
    sc = G.make_scene(scene)
    N = inp["src"].shape[0]
    matches = torch.stack([dev(sc["corr"]), torch.arange(N, device=DEV)], dim=1).contiguous()
    reg = nr.NonRigidRegistration(num_anchors=sc["K"], node_coverage=sc["coverage"], solver="gauss_newton")
    assert reg.num_iterations == 5 and nr.NonRigidRegistration().num_iterations == 500      # each solver's reference default
    warped, T, graph = reg(dev(inp["cloud"]), dev(inp["tgt"]), matches, nodes=dev(inp["nodes"]))
    assert int(graph["status"]) == 0
    assert torch.equal(graph["anchor_indices"], dev(inp["all_ai"]))
    key = "%s_fn_T5" % scene
    want = gold["%s_fn_warp5" % scene]
    assert np.abs(R.apply_deformation(inp["cloud"], inp["nodes"], G.to44(gold[key]), inp["all_ai"], inp["all_aw"]) - want).max() <= 1e-12
    held("%s registration: warped cloud" % scene, warped, want, gold["%s_fn_warp5_dev32" % scene])
    held("%s registration: transforms" % scene, host(T)[:, :3], gold[key], gold[key + "_dev32"])
    # per-match weights are handed on as corr_weights
    reg = nr.NonRigidRegistration(num_anchors=sc["K"], node_coverage=sc["coverage"], num_iterations=5, solver="gauss_newton", arap_lambda=1.0,
                                  lm_lambda=0.01)
    _, T, _ = reg(dev(inp["cloud"]), dev(inp["tgt"]), matches, nodes=dev(inp["nodes"]), match_weights=dev(inp["cw"]))
    held("%s registration with match weights: transforms" % scene, host(T)[:, :3], gold["%s_mod_T5" % scene], gold["%s_mod_T5_dev32" % scene])
    with pytest.raises(ValueError):
        nr.NonRigidRegistration()(dev(inp["cloud"]), dev(inp["tgt"]), matches, nodes=dev(inp["nodes"]), match_weights=dev(inp["cw"]))


# ------------------------------------------------------------------------------------------------ the factor-and-solve alone
def spd_system(n, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, n))
    return g @ g.T + np.eye(n), rng.standard_normal(n)


def backward_error(A, x, b):
    return float(np.linalg.norm(A @ x - b) / (np.linalg.norm(A, 2) * np.linalg.norm(x)))


CANARY = -12345.678


def solve_batch(nr, systems, n_max):
    """the systems in slots of n_max x n_max filled with a canary -> (solutions, slots after the call, right-hand sides after the call, status)"""
    P = len(systems)
    A = np.full((P, n_max, n_max), CANARY)
    b = np.full((P, n_max), CANARY)
    for p, (a, r) in enumerate(systems):
        n = a.shape[0]
        A[p, :n, :n] = np.tril(a) + np.triu(np.full((n, n), CANARY), 1)        # only the lower triangle is the matrix
        b[p, :n] = r
    dA, db = torch.from_numpy(A).to(DEV), torch.from_numpy(b).to(DEV)
    sizes = torch.tensor([a.shape[0] for a, _ in systems], dtype=torch.int32, device=DEV)
    status = nr.spd_solve(dA, db, sizes)
    return host(db), host(dA), host(status)


def check_solution(systems, x, Aout, status, n_max, what):
    for p, (a, r) in enumerate(systems):
        n = a.shape[0]
        assert status[p] == 0
        got = backward_error(a, x[p, :n], r)
        ref = backward_error(a, np.linalg.solve(a, r), r)
        bound = max(n * 2.0 ** -52, 4.0 * ref)
        print("%-28s n %4d: backward error %.3e, numpy's %.3e, bound %.3e" % (what, n, got, ref, bound))
        assert got <= bound
        # what lies outside the system is untouched: the strict upper triangle, the rest of the slot, the rest of the right-hand side
        assert (Aout[p][np.triu_indices(n, 1)] == CANARY).all()
        assert (Aout[p, n:, :] == CANARY).all() and (Aout[p, :, n:] == CANARY).all() and (x[p, n:] == CANARY).all()
        L = np.tril(Aout[p, :n, :n])
        assert np.abs(L @ L.T - a).max() <= 64 * n * 2.0 ** -52 * np.abs(a).max()


@pytest.mark.parametrize("n", (1, 6, B - 1, B, B + 1, 3 * B + 5))
def test_spd_solve_sizes(nr, n):
    systems = [spd_system(n, 100 + n)]
    x, Aout, status = solve_batch(nr, systems, n)
    check_solution(systems, x, Aout, status, n, "alone")
    x2, Aout2, _ = solve_batch(nr, systems, n)
    assert np.array_equal(x, x2) and np.array_equal(Aout, Aout2)
    xs, As, st = solve_batch(nr, systems, n + 7)            # the same system in a wider slot: the same bits
    check_solution(systems, xs, As, st, n + 7, "in a wider slot")
    assert np.array_equal(xs[0, :n], x[0, :n])


def test_spd_solve_batch_of_three_sizes(nr):
    systems = [spd_system(B + 1, 7), spd_system(6, 8), spd_system(3 * B + 5, 9)]
    n_max = 3 * B + 5
    x, Aout, status = solve_batch(nr, systems, n_max)
    check_solution(systems, x, Aout, status, n_max, "batch of three")
    for p, s in enumerate(systems):
        xs, _, _ = solve_batch(nr, [s], n_max)
        assert np.array_equal(xs[0], x[p])


def test_spd_solve_refuses_a_bad_pivot(nr):
    a, r = spd_system(B + 9, 3)
    a[B + 2, B + 2] = -1.0                                   # not positive definite: the pivot of the second block's third column fails
    ok = spd_system(B + 9, 4)
    x, Aout, status = solve_batch(nr, [(a, r), ok], B + 9)
    assert status.tolist() == [32, 0] and np.array_equal(x[0], r) and np.isfinite(Aout[0][np.tril_indices(B + 9)]).all()
    check_solution([ok], x[1:], Aout[1:], status[1:], B + 9, "next to a refused system")


# ------------------------------------------------------------------------------------------------ batch, determinism, capture
def pad_k(inp, K):
    """the same problem with K anchor columns: the added ones are absent (-1, weight 0), which changes no sum"""
    out, n, k = dict(inp), inp["ai"].shape[0], inp["ai"].shape[1]
    out["ai"] = np.concatenate([inp["ai"], np.full((n, K - k), -1, np.int64)], axis=1)
    out["aw"] = np.concatenate([inp["aw"], np.zeros((n, K - k), np.float32)], axis=1)
    return out


def stacked(nr, parts):
    K = max(p["ai"].shape[1] for p in parts)
    parts = [pad_k(p, K) for p in parts]
    cat = lambda k: dev(np.concatenate([p[k] for p in parts]))
    return nr.Problem(cat("nodes"), cat("src"), cat("tgt"), cat("ai"), cat("aw"), cat("edges"), cat("ew"),
                      node_lengths=[p["nodes"].shape[0] for p in parts], corr_lengths=[p["src"].shape[0] for p in parts],
                      edge_lengths=[p["edges"].shape[0] for p in parts])


def without_correspondences(inp):
    out = dict(inp)
    for k in ("src", "tgt", "ai", "aw", "cw"):
        out[k] = inp[k][:0]
    return out


def test_batch_equals_each_pair_alone(nr, gold, runs):
    parts = [G.scene_inputs(gold, "a"), G.scene_inputs(gold, "i"), without_correspondences(G.scene_inputs(gold, "f"))]
    kw = dict(corr_lambda=1.0, arap_lambda=1.0, lm_lambda=0.01)
    cw = dev(np.concatenate([p["cw"] for p in parts]))
    T, status = nr.nicp_gauss_newton(stacked(nr, parts), corr_weights=cw, **kw)
    T2, _ = nr.nicp_gauss_newton(stacked(nr, parts), corr_weights=cw, **kw)
    assert status.tolist() == [0, 0, 0] and torch.equal(T, T2)
    m0 = 0
    for p, name in zip(parts, ("a", "i", None)):
        M = p["nodes"].shape[0]
        solo, st = nr.nicp_gauss_newton(problem_of(nr, p), corr_weights=dev(p["cw"]), **kw)
        assert int(st) == 0 and torch.equal(T[m0:m0 + M], solo)
        if name:
            assert torch.equal(solo, runs[(name, "mod")][5])
        else:                                               # no correspondence: the ARAP residual is zero at the identity, nothing moves
            assert torch.equal(solo, torch.eye(4, device=DEV).expand(M, 4, 4))
        m0 += M


def test_graph_replay_equals_eager(nr, gold, runs):
    inp = G.scene_inputs(gold, "i")
    pb, kw = problem_of(nr, inp), call_args(inp, "mod")
    out = nr.gn_buffers(pb)                                 # transforms, status, workspace: allocated outside the capture
    nr.nicp_gauss_newton(pb, out=out, **kw)                 # uploads the offsets
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            nr.nicp_gauss_newton(pb, out=out, **kw)
    out[0].fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], runs[("i", "mod")][5]) and int(out[1].abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ refusals and edges
def test_unconstrained_node_without_damping_stops_the_pair(nr, gold):
    """lm_lambda = 0 and a node that neither a correspondence nor a non-self edge touches: its pivot is 0"""
    bad = dict(G.scene_inputs(gold, "f"))
    M = bad["nodes"].shape[0]
    bad["nodes"] = np.concatenate([bad["nodes"], np.array([[9.0, 9.0, 9.0]], np.float32)])
    bad["edges"] = np.concatenate([bad["edges"], np.array([[M, M]], np.int64)])
    bad["ew"] = np.concatenate([bad["ew"], np.ones(1, np.float32)])
    ok = G.scene_inputs(gold, "h")
    kw = dict(corr_lambda=1.0, arap_lambda=0.1, lm_lambda=0.0)
    T, status = nr.nicp_gauss_newton(stacked(nr, [bad, ok]), **kw)
    assert status.tolist() == [32, 0]
    assert torch.equal(T[:M + 1], torch.eye(4, device=DEV).expand(M + 1, 4, 4))           # finite, and the starting state
    solo, st = nr.nicp_gauss_newton(problem_of(nr, ok), **kw)
    assert int(st) == 0 and torch.equal(T[M + 1:], solo) and bool(torch.isfinite(T).all())
    # resumed from a state: that state is what comes back
    pb = problem_of(nr, bad)
    state = nr.new_gn_state(pb)
    state["translations"] += 0.25
    before = {k: v.clone() for k, v in state.items()}
    T, status = nr.nicp_gauss_newton(pb, state=state, resume=True, **kw)
    assert int(status) == 32 and torch.equal(state["rotations"], before["rotations"]) and torch.equal(state["translations"], before["translations"])
    assert torch.equal(T[:, :3, 3], before["translations"])


def test_anchor_out_of_range_is_absent(nr, gold):
    inp = dict(G.scene_inputs(gold, "c"))
    M = inp["nodes"].shape[0]
    ai = inp["ai"].copy()
    ai[4, 1], ai[9, 0] = M, M + 5
    inp["ai"] = ai
    T, status = nr.nicp_gauss_newton(problem_of(nr, inp))
    assert int(status) == 4
    ai2 = ai.copy()
    ai2[4, 1], ai2[9, 0] = -1, -1
    inp["ai"] = ai2
    T2, status2 = nr.nicp_gauss_newton(problem_of(nr, inp))
    assert int(status2) == 0 and torch.equal(T, T2)


def test_repeated_anchor_keeps_the_later_column(nr, gold):
    inp = dict(G.scene_inputs(gold, "c"))
    M = inp["nodes"].shape[0]
    ai = inp["ai"].copy()
    ai[7, 0] = ai[7, 2]
    inp["ai"] = ai
    eye, zero = np.tile(np.eye(3), (M, 1, 1)), np.zeros((M, 3))
    A, _, _ = nr.nicp_gn_normal(problem_of(nr, inp), dev(eye), dev(zero))
    want = G.dense(*G.normal_blocks(eye, zero, inp["nodes"], inp["src"], inp["tgt"], ai, inp["aw"], inp["edges"], edge_weights=inp["ew"]))[0]
    held("c with a repeated anchor: A", A[0], want)


def raw_gn(nr, pb, T, status, wsb_delta=0, max_nodes=None):
    from diffreg_hip import lib
    st = pb.struct()
    if max_nodes is not None:
        st2 = lib.NicpProblem()
        ctypes.memmove(ctypes.byref(st2), ctypes.byref(st), ctypes.sizeof(st))
        st2.max_nodes = max_nodes
        st = st2
    op = lib.NicpGnOptions(5, 1.0, 0.1, 0.1)
    wsb = lib.raw().dr_nicp_gn_workspace_bytes(pb.P, pb.n, pb.m, pb.e, pb.K, pb.max_nodes)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    return lib.raw().dr_nicp_gn_f32(ctypes.byref(st), ctypes.byref(op), None, None, 0, lib.ptr(T), lib.ptr(status), lib.ptr(ws), wsb + wsb_delta,
                                    lib.stream_of(T))


def test_refusals(nr, gold, runs):
    inp = G.scene_inputs(gold, "c")
    pb = problem_of(nr, inp)
    M = inp["nodes"].shape[0]
    T = torch.full((M, 4, 4), 7.0, device=DEV)
    status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    assert raw_gn(nr, pb, T, status, wsb_delta=-1) == -4                                  # DR_EWORKSPACE
    assert raw_gn(nr, pb, T, status, max_nodes=1025) == -1                                # DR_EINVAL
    torch.cuda.synchronize()
    assert (T == 7.0).all() and int(status) == 77           # a refused call leaves poisoned outputs as they were
    assert raw_gn(nr, pb, T, status) == 0                   # the size the query states is sufficient
    assert torch.equal(T, runs[("c", "fn")][5]) and int(status) == 0
    # inference only: an input that requires grad raises before any launch
    src = dev(inp["src"]).requires_grad_(True)
    with pytest.raises(RuntimeError, match="requires grad"):
        nr.non_rigid_icp_gauss_newton(dev(inp["nodes"]), src, dev(inp["tgt"]), dev(inp["ai"]), dev(inp["aw"]), dev(inp["edges"]))
    cw = dev(inp["cw"]).requires_grad_(True)
    with pytest.raises(RuntimeError, match="requires grad"):
        nr.nicp_gauss_newton(pb, corr_weights=cw)
    with pytest.raises(RuntimeError, match="requires grad"):
        nr.NonRigidICP()(dev(inp["nodes"]), dev(inp["src"]), dev(inp["tgt"]), dev(inp["ai"]), dev(inp["aw"]).requires_grad_(True),
                         dev(inp["edges"]))
