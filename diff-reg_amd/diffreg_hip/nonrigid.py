"""Non-rigid ICP on an embedded deformation graph (fourteenth set after ABI 0.7.0, csrc/nonrigid.hip): the step from a 4DMatch match
list to a deformation field.

build_euclidean_deformation_graph, apply_deformation and non_rigid_icp_adam keep the names, argument order, defaults and return tuples of
vision3d/ops/deformation_graph.py:26-103, embedded_deformation.py:31-66 and nonrigid_icp_adam.py:76-131; ed_graph, ed_warp, nicp_cost_grad and
nicp_adam are the ragged entries underneath (P pairs per call through offset vectors); NonRigidRegistration chains them behind Pipeline.

Refusals are raised at call time, before any launch: inputs that are not float32, index tensors that are not contiguous int64, a pair with more
nodes than node_capacity().  One exception: when NonRigidRegistration subsamples the nodes itself, their number is known only after that launch,
so the capacity is checked behind it, before the graph and the solver are launched.  There is no CPU path and no path above the capacity.
The ragged entries return the device status vector (the bits are listed in include/diffreg_hip.h); the three vision3d names, whose return tuples
have no place for it, discard it, and NonRigidRegistration hands it out as graph["status"].

The Gauss-Newton solver (sixteenth set, csrc/nonrigid_gn.hip) sits next to the Adam one: non_rigid_icp_gauss_newton and the layer
NonRigidICP keep the signatures of vision3d/layers/nonrigid_icp.py:18-207, nicp_gauss_newton / nicp_gn_normal / spd_solve are the ragged entries,
and NonRigidRegistration(solver="gauss_newton") selects it (the default stays Adam).  It is inference only: an input that requires grad raises.

Furthest-point sampling (seventeenth set, csrc/fps.hip) is where the reference's nodes come from: furthest_point_sample_nodes and
furthest_point_sample keep the signatures of vision3d/array_ops/furthest_point_sample.py:11-19 and vision3d/ops/furthest_point_sample.py:12-49,
fps_nodes is the ragged entry, and NonRigidRegistration(node_sampler="fps") samples its nodes with it (the default stays the grid subsample).

The geodesic graph (eighteenth set, csrc/geo_graph.hip) is the reference's second graph builder: build_deformation_graph_from_point_cloud
keeps the signature and keys of vision3d/array_ops/deformation.py:443-490, geo_graph / geo_graph_edges are the ragged entries, and
NonRigidRegistration(graph="geodesic", node_sampler="fps") takes its anchors and node edges from them (the default stays "euclidean")."""
import ctypes

import torch

from . import lib
from .lib import NicpOptions, NicpProblem, NicpState, check, ptr, stream_of

MAX_ANCHORS = 8
_raw = lib.raw()


def node_capacity():
    """the largest node count of one pair the solver accepts (its state lives in the LDS of one compute unit)"""
    return int(_raw.dr_nicp_node_capacity())


def _f32(name, t, shape_tail):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError("%s must be a float32 tensor (got %s)" % (name, getattr(t, "dtype", type(t))))
    if tuple(t.shape[1:]) != tuple(shape_tail):
        raise ValueError("%s must be [n%s] (got %s)" % (name, "".join(", %d" % s for s in shape_tail), tuple(t.shape)))
    return t.contiguous()


def _i64(name, t, cols):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64:
        raise TypeError("%s must be an int64 tensor (got %s)" % (name, getattr(t, "dtype", type(t))))
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError("%s must be [n, %d] (got %s)" % (name, cols, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _check_k(K):
    if not 1 <= int(K) <= MAX_ANCHORS:
        raise ValueError("num_anchors must be in 1 .. %d (got %s)" % (MAX_ANCHORS, K))
    return int(K)


def _offsets(lengths, dev):
    """host lengths -> (int32 device vector of P + 1 offsets, total); no device read"""
    o = [0]
    for n in lengths:
        o.append(o[-1] + int(n))
    return torch.tensor(o, dtype=torch.int32, device=dev), o[-1]


def _lengths_of(offsets_or_lengths, total):
    """None -> one pair of `total` rows; a list / tuple of host ints -> lengths"""
    if offsets_or_lengths is None:
        return [int(total)]
    lens = [int(n) for n in offsets_or_lengths]
    if sum(lens) != total or min(lens, default=0) < 0:
        raise ValueError("lengths %s do not add up to %d rows" % (lens, total))
    return lens


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


# ------------------------------------------------------------------------------------------------ ragged entries
def ed_graph(points, nodes, num_anchors, node_coverage, point_lengths=None, node_lengths=None, eps=1e-6, return_distance=False):
    """dr_ed_graph_f32 for P pairs: points [n, 3] / nodes [m, 3] stacked, *_lengths host lists (None: one pair).  -> dict(anchor_indices [n, K]
    int64 pair-local (-1 from column min(K, M) on), anchor_weights, anchor_distances?, edge_indices [E, 2] int64 pair-local, edge_weights,
    edge_distances?, edge_lengths (host list), status [P]).  Reads the P edge counts back once, between the count pass and the write pass."""
    points, nodes = _f32("points", points, (3,)), _f32("nodes", nodes, (3,))
    K = _check_k(num_anchors)
    if not float(node_coverage) > 0:
        raise ValueError("node_coverage must be positive")
    pl, ml = _lengths_of(point_lengths, points.shape[0]), _lengths_of(node_lengths, nodes.shape[0])
    if len(pl) != len(ml):
        raise ValueError("point_lengths and node_lengths must describe the same pairs")
    lib.ensure_init()
    dev, P, n, m = points.device, len(pl), points.shape[0], nodes.shape[0]
    po, _ = _offsets(pl, dev)
    mo, _ = _offsets(ml, dev)
    ai = torch.full((n, K), -1, dtype=torch.int64, device=dev)      # a pair the device refuses (status 1 or 2) keeps -1 / 0 rows
    aw = torch.zeros(n, K, device=dev)
    ad = torch.zeros(n, K, device=dev) if return_distance else None
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    mx = max(ml, default=0)
    wsb = _raw.dr_ed_graph_workspace_bytes(m, mx)
    ws = _ws(wsb, dev)
    st = stream_of(points)
    common = (P, n, m, mx, K, ptr(points) if n else None, ptr(po), ptr(nodes) if m else None, ptr(mo), float(node_coverage), float(eps))
    check(_raw.dr_ed_graph_f32(*common, ptr(ai) if n else None, ptr(aw) if n else None, ptr(ad) if (n and return_distance) else None, ptr(counts),
                               None, 0, None, None, None, ptr(status), ptr(ws), wsb, st))
    el = [int(c) for c in counts.tolist()]                  # the one host read of the batch
    eo, E = _offsets(el, dev)
    ei = torch.empty(E, 2, dtype=torch.int64, device=dev)
    ew = torch.empty(E, device=dev)
    edist = torch.empty(E, device=dev) if return_distance else None
    check(_raw.dr_ed_graph_f32(*common, None, None, None, None, ptr(eo), E, ptr(ei) if E else None, ptr(ew) if E else None,
                               ptr(edist) if (E and return_distance) else None, ptr(status), ptr(ws), wsb, st))
    out = dict(anchor_indices=ai, anchor_weights=aw, edge_indices=ei, edge_weights=ew, edge_lengths=el, status=status)
    if return_distance:
        out["anchor_distances"], out["edge_distances"] = ad, edist
    return out


def ed_warp(points, nodes, transforms, anchor_indices, anchor_weights, point_lengths=None, node_lengths=None, eps=1e-6):
    """dr_ed_warp_f32 for P pairs -> (warped [n, 3], status [P])"""
    points, nodes = _f32("points", points, (3,)), _f32("nodes", nodes, (3,))
    transforms = _f32("transforms", transforms, (4, 4))
    if anchor_indices.dim() != 2:
        raise ValueError("anchor_indices must be [n, K]")
    K = _check_k(anchor_indices.shape[1])
    ai = _i64("anchor_indices", anchor_indices, K)
    aw = _f32("anchor_weights", anchor_weights, (K,))
    n, m = points.shape[0], nodes.shape[0]
    if ai.shape[0] != n or aw.shape[0] != n or transforms.shape[0] != m:
        raise ValueError("anchor_indices / anchor_weights need one row per point, transforms one per node")
    pl, ml = _lengths_of(point_lengths, n), _lengths_of(node_lengths, m)
    if len(pl) != len(ml):
        raise ValueError("point_lengths and node_lengths must describe the same pairs")
    lib.ensure_init()
    dev, P = points.device, len(pl)
    po, _ = _offsets(pl, dev)
    mo, _ = _offsets(ml, dev)
    out = torch.empty(n, 3, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    check(_raw.dr_ed_warp_f32(P, n, m, K, ptr(points) if n else None, ptr(po), ptr(nodes) if m else None, ptr(mo), ptr(transforms) if m else None,
                              ptr(ai) if n else None, ptr(aw) if n else None, float(eps), ptr(out) if n else None, ptr(status), stream_of(points)))
    return out, status


class Problem:
    """the inputs of the solver entries for P pairs, validated once: stacked tensors, host lengths, device offsets, the dr_nicp_problem struct"""

    def __init__(self, src_nodes, src_corr_points, tgt_corr_points, anchor_indices, anchor_weights, node_edges, node_edge_weights,
                 node_lengths=None, corr_lengths=None, edge_lengths=None):
        self.nodes = _f32("src_nodes", src_nodes, (3,))
        self.src = _f32("src_corr_points", src_corr_points, (3,))
        self.tgt = _f32("tgt_corr_points", tgt_corr_points, (3,))
        if anchor_indices.dim() != 2:
            raise ValueError("anchor_indices must be [n, K]")
        self.K = _check_k(anchor_indices.shape[1])
        self.ai = _i64("anchor_indices", anchor_indices, self.K)
        self.aw = _f32("anchor_weights", anchor_weights, (self.K,))
        self.edges = _i64("node_edges", node_edges, 2)
        self.ew = _f32("node_edge_weights", node_edge_weights, ())
        self.m, self.n, self.e = self.nodes.shape[0], self.src.shape[0], self.edges.shape[0]
        if self.tgt.shape[0] != self.n or self.ai.shape[0] != self.n or self.aw.shape[0] != self.n or self.ew.shape[0] != self.e:
            raise ValueError("correspondence tensors need one row per correspondence, edge weights one per edge")
        self.ml, self.cl, self.el = _lengths_of(node_lengths, self.m), _lengths_of(corr_lengths, self.n), _lengths_of(edge_lengths, self.e)
        if not len(self.ml) == len(self.cl) == len(self.el):
            raise ValueError("node_lengths, corr_lengths and edge_lengths must describe the same pairs")
        self.P = len(self.ml)
        self.max_nodes = max(self.ml, default=0)
        if self.max_nodes > node_capacity():
            raise ValueError("a pair has %d nodes; the solver holds at most %d (its state lives in one compute unit's LDS)"
                             % (self.max_nodes, node_capacity()))
        self.dev = self.nodes.device
        for t in (self.src, self.tgt, self.ai, self.aw, self.edges, self.ew):
            if t.device != self.dev:
                raise ValueError("all tensors must be on one device")

    def struct(self):
        """built at the first call and kept: the offset vectors are uploaded once, so a later call can be captured in a graph"""
        if getattr(self, "_struct", None) is None:
            self._struct = self._build()
        return self._struct

    def _build(self):
        dev = self.dev
        self.mo, _ = _offsets(self.ml, dev)
        self.co, _ = _offsets(self.cl, dev)
        self.eo, _ = _offsets(self.el, dev)
        v = lambda t, n: ptr(t).value if n else None
        return NicpProblem(self.P, self.n, self.m, self.e, self.K, self.max_nodes, v(self.nodes, self.m), ptr(self.mo).value, v(self.src, self.n),
                           v(self.tgt, self.n), ptr(self.co).value, v(self.ai, self.n), v(self.aw, self.n), v(self.edges, self.e),
                           v(self.ew, self.e), ptr(self.eo).value)

    def workspace(self):
        wsb = _raw.dr_nicp_workspace_bytes(self.P, self.n, self.m, self.e, self.K)
        return _ws(wsb, self.dev), wsb


def nicp_cost_grad(problem, rotations, translations, weights=(1.0, 0.1, 0.1)):
    """dr_nicp_cost_grad_f32 -> (cost [P, 3], grad_rot [m, 3, 3], grad_trn [m, 3], status [P])"""
    rot, trn = _f32("rotations", rotations, (3, 3)), _f32("translations", translations, (3,))
    if rot.shape[0] != problem.m or trn.shape[0] != problem.m:
        raise ValueError("rotations / translations need one row per node")
    lib.ensure_init()
    dev = problem.dev
    pb = problem.struct()
    cost = torch.empty(problem.P, 3, device=dev)
    g_r, g_t = torch.empty_like(rot), torch.empty_like(trn)
    status = torch.empty(problem.P, dtype=torch.int32, device=dev)
    ws, wsb = problem.workspace()
    m = problem.m
    check(_raw.dr_nicp_cost_grad_f32(ctypes.byref(pb), ptr(rot) if m else None, ptr(trn) if m else None, float(weights[0]), float(weights[1]),
                                     float(weights[2]), ptr(cost), ptr(g_r) if m else None, ptr(g_t) if m else None, ptr(status), ptr(ws), wsb,
                                     stream_of(problem.nodes)))
    return cost, g_r, g_t, status


STATE_NAMES = ("rotations", "translations", "exp_avg_rot", "exp_avg_trn", "exp_avg_sq_rot", "exp_avg_sq_trn", "step")


def new_state(problem):
    """an Adam state to run from and to resume: identity rotations, zero translations and moments, step 0"""
    dev, m = problem.dev, problem.m
    z = lambda *s: torch.zeros(*s, device=dev)
    return dict(rotations=torch.eye(3, device=dev).repeat(m, 1, 1), translations=z(m, 3), exp_avg_rot=z(m, 3, 3), exp_avg_trn=z(m, 3),
                exp_avg_sq_rot=z(m, 3, 3), exp_avg_sq_trn=z(m, 3), step=torch.zeros(problem.P, dtype=torch.int32, device=dev))


def nicp_adam(problem, num_iterations=500, lr=0.5, gamma=0.999, beta1=0.9, beta2=0.999, eps=1e-8, weights=(1.0, 0.1, 0.1), state=None,
              resume=False, trace=False, out=None):
    """dr_nicp_adam_f32 -> (transforms [m, 4, 4], cost [P, 3], trace [P, num_iterations, 3] or None, status [P]).  state: a dict of STATE_NAMES
    (new_state()); it receives the final state, and with resume=True the run starts from it.  out: (transforms, cost, trace, status, workspace) of
    an earlier call to write into, so that a captured graph allocates nothing."""
    if int(num_iterations) < 0:
        raise ValueError("num_iterations must not be negative")
    if resume and state is None:
        raise ValueError("resume needs a state")
    lib.ensure_init()
    dev, m, P = problem.dev, problem.m, problem.P
    st = NicpState()
    if state is not None:
        for k in STATE_NAMES:
            t = state.get(k)
            if t is None:
                continue
            want = torch.int32 if k == "step" else torch.float32
            if t.dtype != want or not t.is_contiguous() or t.device != dev or t.numel() != (P if k == "step" else m * (9 if k.endswith("rot") or
                                                                                                                     k == "rotations" else 3)):
                raise ValueError("state[%r] must be a contiguous %s tensor of the problem's size on its device" % (k, want))
            setattr(st, k, ptr(t).value if t.numel() else None)
    pb = problem.struct()
    op = NicpOptions(int(num_iterations), float(lr), float(gamma), float(beta1), float(beta2), float(eps), float(weights[0]), float(weights[1]),
                     float(weights[2]))
    if out is None:
        ws, wsb = problem.workspace()
        out = (torch.empty(m, 4, 4, device=dev), torch.empty(P, 3, device=dev),
               torch.empty(P, int(num_iterations), 3, device=dev) if trace else None, torch.empty(P, dtype=torch.int32, device=dev), ws)
    T, cost, tr, status, ws = out
    wsb = _raw.dr_nicp_workspace_bytes(problem.P, problem.n, problem.m, problem.e, problem.K)
    check(_raw.dr_nicp_adam_f32(ctypes.byref(pb), ctypes.byref(op), ctypes.byref(st), 1 if resume else 0, ptr(T) if m else None, ptr(cost),
                                ptr(tr) if (tr is not None and tr.numel()) else None, ptr(status), ptr(ws), wsb, stream_of(problem.nodes)))
    problem.last_out = out
    return T, cost, tr, status


# ------------------------------------------------------------------------------------------------ Gauss-Newton (sixteenth set)
PIVOT_FAILED = 32        # status bit of the Gauss-Newton entries: a pivot of the factorisation was not finite or not > 0; the pair stopped


def _no_grad(*tensors):
    """the device path is inference only: an input that requires grad is refused before any launch"""
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise RuntimeError("the device Gauss-Newton solver has no backward pass: an input requires grad (detach it)")


def _gn_problem(problem, corr_weights):
    _no_grad(problem.nodes, problem.src, problem.tgt, problem.aw, problem.ew, corr_weights)
    if corr_weights is not None:
        corr_weights = _f32("corr_weights", corr_weights, ())
        if corr_weights.shape[0] != problem.n or corr_weights.device != problem.dev:
            raise ValueError("corr_weights needs one entry per correspondence, on the problem's device")
    return corr_weights


def _gn_workspace_bytes(problem):
    return _raw.dr_nicp_gn_workspace_bytes(problem.P, problem.n, problem.m, problem.e, problem.K, problem.max_nodes)


def gn_buffers(problem):
    """(transforms [m, 4, 4], status [P], workspace) for nicp_gauss_newton(..., out=): allocate once, outside a graph capture or a loop.  The
    workspace is (6 max_nodes)^2 doubles per pair (75 MB at 512 nodes); it lives as long as the caller keeps the tuple."""
    dev = problem.dev
    return (torch.empty(problem.m, 4, 4, device=dev), torch.empty(problem.P, dtype=torch.int32, device=dev),
            _ws(_gn_workspace_bytes(problem), dev))


def _gn_struct(problem, unit_edge_weights):
    """the dr_nicp_problem of a call; edge_weights=None of the reference is a NULL pointer (weight 1)"""
    pb = problem.struct()
    if not unit_edge_weights:
        return pb
    pb2 = lib.NicpProblem()
    ctypes.memmove(ctypes.byref(pb2), ctypes.byref(pb), ctypes.sizeof(pb))
    pb2.edge_weights = None
    return pb2


def new_gn_state(problem):
    """a Gauss-Newton state to run from and to resume: identity rotations, zero translations"""
    return dict(rotations=torch.eye(3, device=problem.dev).repeat(problem.m, 1, 1), translations=torch.zeros(problem.m, 3, device=problem.dev))


def nicp_gauss_newton(problem, num_iterations=5, corr_lambda=1.0, arap_lambda=0.1, lm_lambda=0.1, corr_weights=None, state=None, resume=False,
                      unit_edge_weights=False, out=None):
    """dr_nicp_gn_f32 -> (transforms [m, 4, 4], status [P]).  state: a dict with "rotations" [m, 3, 3] and "translations" [m, 3]
    (new_gn_state()); it receives the final state, and with resume=True the run starts from it.  unit_edge_weights: the reference's
    edge_weights=None.  out: gn_buffers(problem) to write into, so that a captured graph or a loop allocates nothing.
    Inference only: an input that requires grad raises before any launch."""
    if int(num_iterations) < 0:
        raise ValueError("num_iterations must not be negative")
    if resume and state is None:
        raise ValueError("resume needs a state")
    cw = _gn_problem(problem, corr_weights)
    lib.ensure_init()
    dev, m, P = problem.dev, problem.m, problem.P
    st = NicpState()
    if state is not None:
        for k, per in (("rotations", 9), ("translations", 3)):
            t = state.get(k)
            if t is None:
                continue
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or t.numel() != m * per:
                raise ValueError("state[%r] must be a contiguous float32 tensor of the problem's size on its device" % k)
            _no_grad(t)
            setattr(st, k, ptr(t).value if t.numel() else None)
    pb = _gn_struct(problem, unit_edge_weights)
    op = lib.NicpGnOptions(int(num_iterations), float(corr_lambda), float(arap_lambda), float(lm_lambda))
    wsb = _gn_workspace_bytes(problem)
    T, status, ws = gn_buffers(problem) if out is None else out
    if ws.numel() < wsb or T.shape[0] != m or status.numel() != P:
        raise ValueError("out must be gn_buffers() of this problem")
    check(_raw.dr_nicp_gn_f32(ctypes.byref(pb), ctypes.byref(op), ptr(cw) if (cw is not None and problem.n) else None, ctypes.byref(st),
                              1 if resume else 0, ptr(T) if m else None, ptr(status), ptr(ws), wsb, stream_of(problem.nodes)))
    return T, status


def nicp_gn_normal(problem, rotations, translations, corr_lambda=1.0, arap_lambda=0.1, lm_lambda=0.1, corr_weights=None,
                   unit_edge_weights=False):
    """dr_nicp_gn_normal_f32 -> (A [P, 6 max_nodes, 6 max_nodes] float64, b [P, 6 max_nodes] float64, status [P]): the normal equations of ONE
    iteration at the given state; pair p's system is the leading 6 M_p corner of its slot"""
    rot, trn = _f32("rotations", rotations, (3, 3)), _f32("translations", translations, (3,))
    if rot.shape[0] != problem.m or trn.shape[0] != problem.m:
        raise ValueError("rotations / translations need one row per node")
    cw = _gn_problem(problem, corr_weights)
    _no_grad(rot, trn)
    lib.ensure_init()
    dev, m, P, ld = problem.dev, problem.m, problem.P, 6 * problem.max_nodes
    pb = _gn_struct(problem, unit_edge_weights)
    op = lib.NicpGnOptions(1, float(corr_lambda), float(arap_lambda), float(lm_lambda))
    A = torch.empty(P, ld, ld, dtype=torch.float64, device=dev)
    b = torch.empty(P, ld, dtype=torch.float64, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    wsb = _gn_workspace_bytes(problem)
    ws = _ws(wsb, dev)
    check(_raw.dr_nicp_gn_normal_f32(ctypes.byref(pb), ctypes.byref(op), ptr(cw) if (cw is not None and problem.n) else None,
                                     ptr(rot) if m else None, ptr(trn) if m else None, ptr(A) if A.numel() else None,
                                     ptr(b) if b.numel() else None, ptr(status), ptr(ws), wsb, stream_of(problem.nodes)))
    return A, b, status


def spd_solve(A, b, sizes=None):
    """dr_spd_solve_f64, IN PLACE: A [P, n_max, n_max] float64 (lower triangle read; receives the Cholesky factor), b [P, n_max] float64
    (receives the solution); sizes: int32 device tensor [P] of each system's n (None: all n_max).  -> status [P] (32: a pivot was not > 0)"""
    if A.dtype != torch.float64 or b.dtype != torch.float64 or A.dim() != 3 or A.shape[1] != A.shape[2] or tuple(b.shape) != tuple(A.shape[:2]):
        raise ValueError("A must be [P, n, n] float64 and b [P, n] float64")
    if not (A.is_contiguous() and b.is_contiguous()) or A.device != b.device:
        raise ValueError("A and b must be contiguous and on one device")
    lib.ensure_init()
    P, n = A.shape[0], A.shape[1]
    if sizes is None:
        sizes = torch.full((P,), n, dtype=torch.int32, device=A.device)
    if sizes.dtype != torch.int32 or sizes.numel() != P or sizes.device != A.device or not sizes.is_contiguous():
        raise ValueError("sizes must be a contiguous int32 tensor [P] on A's device")
    status = torch.empty(P, dtype=torch.int32, device=A.device)
    check(_raw.dr_spd_solve_f64(P, n, ptr(sizes) if P else None, ptr(A) if A.numel() else None, ptr(b) if b.numel() else None,
                                ptr(status) if P else None, stream_of(A)))
    return status


# ------------------------------------------------------------------------------------------------ furthest-point sampling (seventeenth set)
FPS_CAP_REACHED = 64       # status bit of fps_nodes: sample_cap nodes were taken before the stop rule was met
FPS_START_NONFINITE = 128  # status bit of fps_nodes: point 0 of the cloud is not finite, the cloud yields 0 nodes


def _device_tensor(name, t):
    """the new public names refuse a host tensor: its data pointer would be handed to the kernel as a device address"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s must be a tensor on the GPU (got %s)" % (name, getattr(t, "device", type(t))))


def fps_onchip_capacity():
    """the largest cloud whose coordinates and running distances stay in registers; a larger one takes the streaming form of the same kernel"""
    return int(_raw.dr_fps_onchip_capacity())


def fps_nodes(points, min_distance=None, num_samples=None, lengths=None, sample_cap=None, return_distance=False, out=None):
    """dr_fps_nodes_f32 for P clouds: points [n, 3] stacked, lengths a host list (None: one cloud).  min_distance / num_samples: the stop rules of
    vision3d's array_ops.furthest_point_sample (None: absent; at least one is needed, and min_distance <= 0 counts as absent).  sample_cap: the
    row length of the outputs (default: num_samples, else the largest cloud).  Reads nothing back.  -> dict(indices [P, sample_cap] int64
    cloud-local, -1 beyond the count; points [P, sample_cap, 3]; distances [P, sample_cap] when return_distance: the running-minimum distance
    at which each node was taken; counts [P] int32; status [P] int32; offsets, workspace).  out: the dict of an earlier call of the same
    shapes to write into, so that a captured graph allocates and uploads nothing."""
    points = _f32("points", points, (3,))
    lens = _lengths_of(lengths, points.shape[0])
    md = -1.0 if min_distance is None else float(min_distance)
    ns = -1 if num_samples is None else int(num_samples)
    if num_samples is not None and ns < 1:
        raise ValueError("num_samples must be positive (got %s)" % (num_samples,))
    if not md > 0 and ns <= 0:
        raise ValueError("furthest-point sampling needs min_distance > 0 or num_samples: with neither the reference's loop cannot stop")
    P, n, mx = len(lens), points.shape[0], max(lens, default=0)
    cap = int(sample_cap) if sample_cap is not None else (ns if ns > 0 else max(mx, 1))
    if cap < 1:
        raise ValueError("sample_cap must be positive (got %s)" % (sample_cap,))
    _device_tensor("points", points)
    lib.ensure_init()
    dev = points.device
    wsb = _raw.dr_fps_workspace_bytes(P, n, mx)
    if out is None:
        out = dict(indices=torch.empty(P, cap, dtype=torch.int64, device=dev), points=torch.empty(P, cap, 3, device=dev),
                   counts=torch.empty(P, dtype=torch.int32, device=dev), status=torch.empty(P, dtype=torch.int32, device=dev),
                   offsets=_offsets(lens, dev)[0], workspace=_ws(wsb, dev), lengths=lens)
        if return_distance:
            out["distances"] = torch.empty(P, cap, device=dev)
    elif tuple(out["indices"].shape) != (P, cap) or out["lengths"] != lens or out["workspace"].numel() < wsb or (return_distance and
                                                                                                               "distances" not in out):
        raise ValueError("out must be the result of an earlier call with the same lengths, sample_cap and return_distance")
    check(_raw.dr_fps_nodes_f32(P, n, mx, ptr(points) if n else None, ptr(out["offsets"]), md, ns, cap, ptr(out["indices"]) if P else None,
                                ptr(out["points"]) if P else None, ptr(out["distances"]) if (P and return_distance) else None,
                                ptr(out["counts"]) if P else None, ptr(out["status"]) if P else None, ptr(out["workspace"]), wsb,
                                stream_of(points)))
    return out


def furthest_point_sample_nodes(points, min_distance=None, num_samples=None):
    """vision3d/array_ops/furthest_point_sample.py:11-19 for one cloud on the device -> int64 indices [count] (one host read: the count).
    Ties go to the lowest index and a non-finite point is never taken (include/diffreg_hip.h); the status word is discarded (fps_nodes
    returns it)."""
    r = fps_nodes(points, min_distance=min_distance, num_samples=num_samples)
    return r["indices"][0, :int(r["counts"][0])].clone()


def furthest_point_sample(points, num_samples, *input_tensors, gather_points=True, transposed=False):
    """vision3d/ops/furthest_point_sample.py:12-49: points [B, N, 3] ([B, 3, N] when transposed), features [B, C, N] -> indices [B, M] when
    not gather_points, else (sampled_points [B, M, 3] or [B, 3, M], *sampled features [B, C, M]), as the reference returns them."""
    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() != 3:
        raise TypeError("points must be a float32 tensor [B, N, 3]")
    _device_tensor("points", points)         # input_tensors only pass through torch.gather, which checks its own devices
    if transposed:
        points = points.transpose(1, 2)
    points = points.contiguous()
    if points.shape[2] != 3:
        raise ValueError("points must be [B, N, 3] (got %s)" % (tuple(points.shape),))
    B, N, M = points.shape[0], points.shape[1], int(num_samples)
    if M < 0 or (N == 0 and M > 0 and B > 0):
        raise ValueError("num_samples must not be negative, and an empty cloud has no sample")
    lib.ensure_init()
    indices = torch.zeros(B, M, dtype=torch.int64, device=points.device)
    if B and M:
        wsb = _raw.dr_fps_workspace_bytes(B, B * N, N)
        ws = _ws(wsb, points.device)
        check(_raw.dr_fps_batch_f32(B, N, M, ptr(points), ptr(indices), ptr(ws), wsb, stream_of(points)))
    if not gather_points:
        return indices
    sampled = torch.gather(points, 1, indices[:, :, None].expand(B, M, 3))
    if transposed:
        sampled = sampled.transpose(1, 2).contiguous()
    outs = [torch.gather(t, 2, indices[:, None, :].expand(B, t.shape[1], M)) for t in input_tensors]
    return (sampled, *outs)


# ------------------------------------------------------------------------------------------------ geodesic graph (eighteenth set)
GEO_MAX_K = 8              # compiled limit of num_neighbors and num_anchors
GEO_DUPLICATE_NODE = 256   # status bit of geo_graph: two nodes name one point; the cloud's results are only guaranteed to be in range
GEO_DEGREE_OVERFLOW = 512  # status bit of geo_graph: a point has more than max_degree points closer than max_distance; rows of padding only


def geo_graph_onchip_capacity():
    """the largest cloud whose path lengths stay in LDS while a node relaxes them; a larger one relaxes in the workspace, with the same result"""
    return int(_raw.dr_geo_graph_onchip_capacity())


def geo_graph(points, node_indices, num_neighbors, num_anchors, max_distance, node_coverage, point_lengths=None, node_lengths=None,
              max_degree=64, onchip_cap_override=0, out=None):
    """dr_geo_graph_f32 for P clouds: vision3d's build_deformation_graph_from_point_cloud on the device.  points [n, 3] stacked, node_indices [m]
    int64 CLOUD-LOCAL point indices (as fps_nodes returns them), *_lengths host lists (None: one cloud).  Points closer than max_distance are
    joined; a node reaches what lies within 2 node_coverage of it ALONG that graph.  -> dict(neighbor_indices [m, Kn] int64 cloud-local node
    numbers, neighbor_distances, neighbor_weights, anchor_indices [n, Ka], anchor_distances, anchor_weights, status [P]; offsets, workspace).
    Rows are padded with -1 / 0 / 0; a point no node reaches has a whole row of padding.  max_degree: the slots of a point's adjacency row in
    the workspace; a cloud with a denser point gets GEO_DEGREE_OVERFLOW and padding only.  Reads nothing back.  out: the dict of an earlier
    call of the same shapes to write into, so that a captured graph allocates and uploads nothing."""
    points = _f32("points", points, (3,))
    if not isinstance(node_indices, torch.Tensor) or node_indices.dtype != torch.int64 or node_indices.dim() != 1:
        raise TypeError("node_indices must be a 1-d int64 tensor (got %s)" % (getattr(node_indices, "dtype", type(node_indices)),))
    Kn, Ka = int(num_neighbors), int(num_anchors)
    if not 1 <= Kn <= GEO_MAX_K or not 1 <= Ka <= GEO_MAX_K:
        raise ValueError("num_neighbors and num_anchors must be in 1 .. %d (got %s, %s)" % (GEO_MAX_K, num_neighbors, num_anchors))
    if not (float(max_distance) > 0 and float(node_coverage) > 0):
        raise ValueError("max_distance and node_coverage must be positive")
    if not 1 <= int(max_degree) <= 1024 or int(onchip_cap_override) < 0:
        raise ValueError("max_degree must be in 1 .. 1024 and onchip_cap_override must not be negative")
    node_indices = node_indices.contiguous()
    pl, ml = _lengths_of(point_lengths, points.shape[0]), _lengths_of(node_lengths, node_indices.shape[0])
    if len(pl) != len(ml):
        raise ValueError("point_lengths and node_lengths must describe the same clouds")
    _device_tensor("points", points)
    _device_tensor("node_indices", node_indices)
    lib.ensure_init()
    dev, P, n, m, mxp, mxn = points.device, len(pl), points.shape[0], node_indices.shape[0], max(pl, default=0), max(ml, default=0)
    wsb = _raw.dr_geo_graph_workspace_bytes(P, n, m, mxp, int(max_degree))
    if out is None:
        f = lambda r, k: torch.zeros(r, k, device=dev)
        out = dict(neighbor_indices=torch.full((m, Kn), -1, dtype=torch.int64, device=dev), neighbor_distances=f(m, Kn), neighbor_weights=f(m, Kn),
                   anchor_indices=torch.full((n, Ka), -1, dtype=torch.int64, device=dev), anchor_distances=f(n, Ka), anchor_weights=f(n, Ka),
                   status=torch.empty(P, dtype=torch.int32, device=dev), offsets=(_offsets(pl, dev)[0], _offsets(ml, dev)[0]),
                   workspace=_ws(wsb, dev), lengths=(pl, ml))
    elif (tuple(out["neighbor_indices"].shape) != (m, Kn) or tuple(out["anchor_indices"].shape) != (n, Ka) or out["lengths"] != (pl, ml)
          or out["workspace"].numel() < wsb):
        raise ValueError("out must be the result of an earlier call with the same lengths, num_neighbors, num_anchors and max_degree")
    op = lib.GeoGraphOptions(Kn, Ka, float(max_distance), float(node_coverage), int(max_degree), int(onchip_cap_override))
    v = lambda t, k: ptr(t) if k else None
    check(_raw.dr_geo_graph_f32(P, n, m, mxp, mxn, v(points, n), ptr(out["offsets"][0]), v(node_indices, m), ptr(out["offsets"][1]),
                                ctypes.byref(op), v(out["neighbor_indices"], m), v(out["neighbor_distances"], m), v(out["neighbor_weights"], m),
                                v(out["anchor_indices"], n), v(out["anchor_distances"], n), v(out["anchor_weights"], n),
                                ptr(out["status"]) if P else None, ptr(out["workspace"]), wsb, stream_of(points)))
    return out


def geo_graph_edges(neighbor_indices, neighbor_weights, node_lengths=None):
    """dr_geo_graph_edges: the neighbour table as the edge list Problem takes -- edge (i, j) for every valid neighbour j != i of node i, in
    row-major order, with the neighbour's weight.  -> (edge_indices [E, 2] int64 cloud-local, edge_weights [E], edge_lengths host list).  Reads
    the P edge counts back once, between the count pass and the write pass, as ed_graph does."""
    if neighbor_indices.dim() != 2:
        raise ValueError("neighbor_indices must be [m, Kn]")
    Kn = neighbor_indices.shape[1]
    if not 1 <= Kn <= GEO_MAX_K:
        raise ValueError("num_neighbors must be in 1 .. %d (got %s)" % (GEO_MAX_K, Kn))
    ni, nw = _i64("neighbor_indices", neighbor_indices, Kn), _f32("neighbor_weights", neighbor_weights, (Kn,))
    _device_tensor("neighbor_indices", ni)
    _device_tensor("neighbor_weights", nw)
    m = ni.shape[0]
    if nw.shape[0] != m:
        raise ValueError("neighbor_weights needs one row per node")
    ml = _lengths_of(node_lengths, m)
    lib.ensure_init()
    dev, P, st = ni.device, len(ml), stream_of(ni)
    mo, _ = _offsets(ml, dev)
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    check(_raw.dr_geo_graph_edges(P, m, Kn, ptr(ni) if m else None, ptr(nw) if m else None, ptr(mo), ptr(counts), None, 0, None, None, st))
    el = [int(c) for c in counts.tolist()]                  # the one host read of the batch
    eo, E = _offsets(el, dev)
    ei = torch.empty(E, 2, dtype=torch.int64, device=dev)
    ew = torch.empty(E, device=dev)
    check(_raw.dr_geo_graph_edges(P, m, Kn, ptr(ni) if m else None, ptr(nw) if m else None, ptr(mo), None, ptr(eo), E, ptr(ei) if E else None,
                                  ptr(ew) if E else None, st))
    return ei, ew, el


def build_deformation_graph_from_point_cloud(points, node_indices, num_neighbors, num_anchors, max_distance, node_coverage):
    """vision3d/array_ops/deformation.py:443-490 for one cloud on the device -> the reference's six keys.  The status word is discarded
    (geo_graph returns it).  Each point's anchors stand in the point's own row (the reference writes the r-th reached point's into row r)."""
    g = geo_graph(points, node_indices, num_neighbors, num_anchors, max_distance, node_coverage)
    return {k: g[k] for k in ("neighbor_indices", "neighbor_distances", "neighbor_weights", "anchor_indices", "anchor_distances",
                              "anchor_weights")}


# ------------------------------------------------------------------------------------------------ vision3d's three names
def build_euclidean_deformation_graph(points, nodes, num_anchors, node_coverage, return_point_anchor=True, return_node_graph=True,
                                      return_distance=False, return_adjacent_matrix=False, eps=1e-6):
    """vision3d/ops/deformation_graph.py:26-103 for one pair; the anchor tensors have min(num_anchors, M) columns, as the reference's.  The
    reference's tuple has no place for the device status word, so it is DISCARDED here (ed_graph returns it): with points but no nodes the anchors
    are -1 / weight 0, and a NaN / Inf coordinate leaves -1 columns where the reference returns NaN weights."""
    if return_adjacent_matrix:
        raise NotImplementedError("return_adjacent_matrix=True: the device builds the edge list, not the dense matrices")
    g = ed_graph(points, nodes, num_anchors, node_coverage, eps=eps, return_distance=return_distance)
    ke = min(int(num_anchors), nodes.shape[0])
    cut = (lambda t: t[:, :ke].contiguous()) if ke < int(num_anchors) else (lambda t: t)
    out = []
    if return_point_anchor:
        out += [cut(g["anchor_indices"]), cut(g["anchor_weights"])]
        if return_distance:
            out.append(cut(g["anchor_distances"]))
    if return_node_graph:
        out += [g["edge_indices"], g["edge_weights"]]
        if return_distance:
            out.append(g["edge_distances"])
    return tuple(out)


def apply_deformation(points, nodes, transforms, anchor_indices, anchor_weights, eps=1e-6):
    """vision3d/ops/embedded_deformation.py:31-66 for one pair; the status word is discarded (ed_warp returns it): an anchor outside [-1, M) is
    treated as absent where the reference raises an IndexError"""
    return ed_warp(points, nodes, transforms, anchor_indices, anchor_weights, eps=eps)[0]


def non_rigid_icp_adam(src_nodes, src_corr_points, tgt_corr_points, anchor_indices, anchor_weights, node_edges, node_edge_weights,
                       num_iterations=500):
    """vision3d/ops/nonrigid_icp_adam.py:76-131 for one pair -> transforms [M, 4, 4]; the status word is discarded (nicp_adam returns it)"""
    pb = Problem(src_nodes, src_corr_points, tgt_corr_points, anchor_indices, anchor_weights, node_edges, node_edge_weights)
    return nicp_adam(pb, num_iterations=num_iterations)[0]


def non_rigid_icp_gauss_newton(src_nodes, src_corr_points, tgt_corr_points, anchor_indices, anchor_weights, edge_indices, corr_weights=None,
                               edge_weights=None, corr_lambda=1.0, arap_lambda=0.1, lm_lambda=0.1, num_iterations=5):
    """vision3d/layers/nonrigid_icp.py:18-154 for one pair -> transforms [M, 4, 4]; the status word is discarded (nicp_gauss_newton returns it).
    Inference only: an input that requires grad raises.  A row that names one node in two columns keeps the later column's Jacobian block."""
    _no_grad(src_nodes, src_corr_points, tgt_corr_points, anchor_weights, corr_weights, edge_weights)
    unit = edge_weights is None
    if unit:
        edge_weights = torch.ones(edge_indices.shape[0], device=src_nodes.device)
    pb = Problem(src_nodes, src_corr_points, tgt_corr_points, anchor_indices, anchor_weights, edge_indices, edge_weights)
    return nicp_gauss_newton(pb, num_iterations=num_iterations, corr_lambda=corr_lambda, arap_lambda=arap_lambda, lm_lambda=lm_lambda,
                             corr_weights=corr_weights, unit_edge_weights=unit)[0]


class NonRigidICP(torch.nn.Module):
    """vision3d/layers/nonrigid_icp.py:157-207: the Gauss-Newton solver as a layer (inference only)"""

    def __init__(self, corr_lambda=1.0, arap_lambda=1.0, lm_lambda=0.01, num_iterations=5):
        super().__init__()
        self.corr_lambda, self.arap_lambda, self.lm_lambda, self.num_iterations = corr_lambda, arap_lambda, lm_lambda, num_iterations

    def forward(self, src_nodes, src_corr_points, tgt_corr_points, anchor_indices, anchor_weights, edge_indices, corr_weights=None,
                edge_weights=None):
        return non_rigid_icp_gauss_newton(src_nodes, src_corr_points, tgt_corr_points, anchor_indices, anchor_weights, edge_indices,
                                          corr_weights=corr_weights, edge_weights=edge_weights, corr_lambda=self.corr_lambda,
                                          arap_lambda=self.arap_lambda, lm_lambda=self.lm_lambda, num_iterations=self.num_iterations)

    def extra_repr(self):
        return ", ".join(["corr_lambda=%g" % self.corr_lambda, "arap_lambda=%g" % self.arap_lambda, "lm_lambda=%g" % self.lm_lambda,
                          "num_iterations=%d" % self.num_iterations])


# ------------------------------------------------------------------------------------------------ after Pipeline on a 4DMatch pair
class NonRigidRegistration:
    """graph -> solver -> warp of the whole source cloud, for one pair or a list of pairs in one call.

    __call__(src_points, tgt_points, matches, nodes=None): src_points [n, 3] / tgt_points [n', 3] float32, matches [k, 2] int64 (source row,
    target row) as Pipeline returns them per pair -- or lists of those, one entry per pair.  nodes: given per pair, or grid-subsampled from the
    source cloud with cell = node_coverage (dr_grid_subsample_f32).  -> (warped_src, transforms, graph) per pair (lists for a list).
    graph["status"] is the pair's device status word (a 0-d int32 DEVICE tensor, not read here: 0, or the bits include/diffreg_hip.h lists --
    8: a non-finite coordinate left points without their full anchors; 4: an index out of range was treated as absent)."""

    def __init__(self, num_anchors=6, node_coverage=0.08, num_iterations=None, lr=0.5, gamma=0.999, weights=(1.0, 0.1, 0.1), eps=1e-6,
                 solver="adam", corr_lambda=1.0, arap_lambda=0.1, lm_lambda=0.1, node_sampler="grid", node_min_distance=None,
                 graph="euclidean", num_neighbors=8, max_distance=None, max_degree=64):
        """solver="gauss_newton": dr_nicp_gn_f32 with the three lambdas in place of the Adam solver; __call__ then takes match_weights,
        per-match weights handed on as corr_weights.  num_iterations=None is each solver's reference default: 500 (Adam), 5 (Gauss-Newton).
        node_sampler: where the nodes come from when __call__ is given none -- "grid" (the default): grid barycentres with cell =
        node_coverage; "fps": furthest-point sampling as vision3d's array_ops.furthest_point_sample, with min_distance = node_min_distance
        (None: node_coverage) and node_capacity() as the cap: the nodes are points of the cloud, at least min_distance apart, never more than
        the solver holds; a pair cut by the cap carries FPS_CAP_REACHED in graph["status"].
        graph: "euclidean" (the default): anchors are the nearest nodes in space (ed_graph); "geodesic": anchors and node edges come from
        geo_graph, i.e. from path lengths along the cloud's own point graph (points closer than max_distance are joined; None: node_coverage
        / 2), with num_neighbors neighbours per node, so that two surfaces that are close without being connected do not share nodes.  The
        nodes must then be points of the cloud: it requires node_sampler="fps" (whose indices are used), or __call__'s node_indices=.
        ed_warp sends a point whose anchors are all -1 to the origin, as the reference's apply_deformation does; under "geodesic" a point
        that no node reaches has such a row, and __call__ LEAVES IT WHERE IT IS (it copies the source coordinates into those rows).  A cloud
        with GEO_DEGREE_OVERFLOW in graph["status"] has no anchors at all: raise max_degree."""
        if graph not in ("euclidean", "geodesic"):
            raise ValueError("graph must be 'euclidean' or 'geodesic' (got %r)" % (graph,))
        if graph == "geodesic" and node_sampler != "fps":
            raise ValueError("graph='geodesic' needs nodes that are points of the cloud: construct with node_sampler='fps'")
        self.graph, self.num_neighbors, self.max_degree = graph, int(num_neighbors), int(max_degree)
        if graph == "geodesic" and not 1 <= self.num_neighbors <= GEO_MAX_K:
            raise ValueError("num_neighbors must be in 1 .. %d (got %s)" % (GEO_MAX_K, num_neighbors))
        self.max_distance = float(node_coverage) / 2 if max_distance is None else float(max_distance)
        if graph == "geodesic" and not self.max_distance > 0:
            raise ValueError("max_distance must be positive")
        if solver not in ("adam", "gauss_newton"):
            raise ValueError("solver must be 'adam' or 'gauss_newton' (got %r)" % (solver,))
        if node_sampler not in ("grid", "fps"):
            raise ValueError("node_sampler must be 'grid' or 'fps' (got %r)" % (node_sampler,))
        self.node_sampler = node_sampler
        self.node_min_distance = float(node_coverage if node_min_distance is None else node_min_distance)
        if node_sampler == "fps" and not self.node_min_distance > 0:
            raise ValueError("node_min_distance must be positive")
        if num_iterations is None:
            num_iterations = 500 if solver == "adam" else 5
        self.num_anchors, self.node_coverage, self.num_iterations = _check_k(num_anchors), float(node_coverage), int(num_iterations)
        self.lr, self.gamma, self.weights, self.eps = float(lr), float(gamma), tuple(weights), float(eps)
        self.solver, self.corr_lambda, self.arap_lambda, self.lm_lambda = solver, float(corr_lambda), float(arap_lambda), float(lm_lambda)

    def subsample_nodes(self, src_list):
        """per-pair node sets: one grid-subsample call over the stacked clouds, one host read of the P lengths"""
        dev = src_list[0].device
        lengths = torch.tensor([s.shape[0] for s in src_list], dtype=torch.int32, device=dev)
        pts, sub_len, _, _ = lib.grid_subsample(torch.cat(src_list), lengths, self.node_coverage)
        out, lo = [], 0
        for n in sub_len.tolist():
            out.append(pts[lo:lo + n].contiguous())
            lo += n
        return out

    def sample_nodes_fps(self, src_list):
        """per-pair node sets by furthest-point sampling: one ragged call over the stacked clouds, one host read of the P counts.
        -> (list of [count, 3] node tensors, status [P] on the device)"""
        r = fps_nodes(torch.cat(src_list), min_distance=self.node_min_distance, lengths=[s.shape[0] for s in src_list],
                      sample_cap=node_capacity())
        counts = r["counts"].tolist()
        self._fps_indices = [r["indices"][p, :c].contiguous() for p, c in enumerate(counts)]
        return [r["points"][p, :c].contiguous() for p, c in enumerate(counts)], r["status"]

    def __call__(self, src_points, tgt_points, matches, nodes=None, match_weights=None, node_indices=None):
        """node_indices (graph="geodesic" only): per pair the int64 rows of the source cloud that are its nodes, in place of sampling them"""
        single = isinstance(src_points, torch.Tensor)
        if match_weights is not None and self.solver != "gauss_newton":
            raise ValueError("match_weights are the Gauss-Newton solver's corr_weights: construct with solver='gauss_newton'")
        src_l = [src_points] if single else list(src_points)
        tgt_l = [tgt_points] if single else list(tgt_points)
        mat_l = [matches] if single else list(matches)
        nod_l = None if nodes is None else ([nodes] if single else list(nodes))
        if not len(src_l) == len(tgt_l) == len(mat_l) or (nod_l is not None and len(nod_l) != len(src_l)):
            raise ValueError("one source cloud, target cloud, match list (and node set) per pair")
        idx_l = None
        if node_indices is not None:
            if self.graph != "geodesic" or nodes is not None:
                raise ValueError("node_indices belong to graph='geodesic' and replace nodes=")
            idx_l = [node_indices] if single else list(node_indices)
            if len(idx_l) != len(src_l):
                raise ValueError("one node index list per pair")
            nod_l = [s[i] for s, i in zip(src_l, idx_l)]
        elif self.graph == "geodesic" and nodes is not None:
            raise ValueError("graph='geodesic' needs the nodes as rows of the source cloud: pass node_indices=, not nodes=")
        src_l = [_f32("src_points", s, (3,)) for s in src_l]
        tgt_l = [_f32("tgt_points", t, (3,)) for t in tgt_l]
        mat_l = [_i64("matches", m, 2) for m in mat_l]
        if nod_l is not None:
            nod_l = [_f32("nodes", g, (3,)) for g in nod_l]
            if max(g.shape[0] for g in nod_l) > node_capacity():
                raise ValueError("a pair has %d nodes; the solver holds at most %d" % (max(g.shape[0] for g in nod_l), node_capacity()))
        st_nodes = None
        if nod_l is None and self.node_sampler == "fps":
            nod_l, st_nodes = self.sample_nodes_fps(src_l)       # at most node_capacity() nodes per pair, by the call's sample_cap
            idx_l = self._fps_indices
        elif nod_l is None:
            nod_l = self.subsample_nodes(src_l)      # a launch: only now is the node count known, so the capacity is checked here,
            if max(g.shape[0] for g in nod_l) > node_capacity():                     # before the graph and the solver are launched
                raise ValueError("the grid subsample gave a pair %d nodes; the solver holds at most %d: raise node_coverage or pass nodes"
                                 % (max(g.shape[0] for g in nod_l), node_capacity()))
        pl, ml, cl = [s.shape[0] for s in src_l], [g.shape[0] for g in nod_l], [m.shape[0] for m in mat_l]
        src, nod = torch.cat(src_l), torch.cat(nod_l)
        if self.graph == "geodesic":
            gg = geo_graph(src, torch.cat(idx_l), self.num_neighbors, self.num_anchors, self.max_distance, self.node_coverage,
                           point_lengths=pl, node_lengths=ml, max_degree=self.max_degree)
            ei, ew, el = geo_graph_edges(gg["neighbor_indices"], gg["neighbor_weights"], node_lengths=ml)
            g = dict(anchor_indices=gg["anchor_indices"], anchor_weights=gg["anchor_weights"], edge_indices=ei, edge_weights=ew, edge_lengths=el,
                     status=gg["status"] & ~3)          # its 1 and 2 mean other things than this word's
        else:
            g = ed_graph(src, nod, self.num_anchors, self.node_coverage, point_lengths=pl, node_lengths=ml, eps=self.eps)
        rows, lo = [], 0
        for s, m in zip(src_l, mat_l):                      # the correspondences' rows of the stacked source cloud
            rows.append(m[:, 0] + lo)
            lo += s.shape[0]
        rows = torch.cat(rows)
        src_corr = src[rows]
        tgt_corr = torch.cat([t[m[:, 1]] for t, m in zip(tgt_l, mat_l)])
        pb = Problem(nod, src_corr, tgt_corr, g["anchor_indices"][rows].contiguous(), g["anchor_weights"][rows].contiguous(), g["edge_indices"],
                     g["edge_weights"], node_lengths=ml, corr_lengths=cl, edge_lengths=g["edge_lengths"])
        if self.solver == "gauss_newton":
            cw = None
            if match_weights is not None:
                cw_l = [match_weights] if single else list(match_weights)
                if len(cw_l) != len(mat_l) or any(w.shape[0] != m.shape[0] for w, m in zip(cw_l, mat_l)):
                    raise ValueError("one weight per match")
                cw = torch.cat([_f32("match_weights", w, ()) for w in cw_l])
            T, st_solver = nicp_gauss_newton(pb, num_iterations=self.num_iterations, corr_lambda=self.corr_lambda,
                                             arap_lambda=self.arap_lambda, lm_lambda=self.lm_lambda, corr_weights=cw)
        else:
            T, _, _, st_solver = nicp_adam(pb, num_iterations=self.num_iterations, lr=self.lr, gamma=self.gamma, weights=self.weights)
        warped, st_warp = ed_warp(src, nod, T, g["anchor_indices"], g["anchor_weights"], point_lengths=pl, node_lengths=ml, eps=self.eps)
        if self.graph == "geodesic":                     # a point no node reaches stays where it is (ed_warp alone sends it to the origin)
            warped = torch.where((g["anchor_indices"] >= 0).any(1, keepdim=True), warped, src)
        st_all = g["status"] | st_solver | st_warp
        if st_nodes is not None:
            st_all = st_all | (st_nodes & (FPS_CAP_REACHED | FPS_START_NONFINITE))   # the sampler's 1 / 2 / 8 mean other things than this word's
        res, p0, m0, e0 = [], 0, 0, 0
        for p, m, e in zip(pl, ml, g["edge_lengths"]):
            graph = dict(nodes=nod[m0:m0 + m], anchor_indices=g["anchor_indices"][p0:p0 + p], anchor_weights=g["anchor_weights"][p0:p0 + p],
                         edge_indices=g["edge_indices"][e0:e0 + e], edge_weights=g["edge_weights"][e0:e0 + e],
                         status=st_all[len(res)])
            res.append((warped[p0:p0 + p], T[m0:m0 + m], graph))
            p0, m0, e0 = p0 + p, m0 + m, e0 + e
        return res[0] if single else ([r[0] for r in res], [r[1] for r in res], [r[2] for r in res])

    def evaluate(self, result, src_points, scene_flows, tgt_points, gt_transform=None, matches=None, test_indices=None, **kw):
        """__call__'s output, for one pair or a list of pairs, into metrics_nonrigid.evaluate_nonrigid_pairs (which names the keyword
        arguments: the strict / relaxed / outlier threshold pairs are required); -> its dict.  Nothing is read back."""
        from . import metrics_nonrigid
        single = isinstance(src_points, torch.Tensor)
        wrap = (lambda x: None if x is None else [x]) if single else (lambda x: None if x is None else list(x))
        return metrics_nonrigid.evaluate_nonrigid_pairs(wrap(src_points), wrap(result[0]), wrap(scene_flows), wrap(tgt_points),
                                                        wrap(gt_transform), wrap(matches), wrap(test_indices), **kw)
