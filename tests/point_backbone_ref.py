"""Test-side float64 statement of the point-convolution primitives under both backbones (csrc/backbone.hip, csrc/backbone_bwd.hip and the
kNN-interpolation / neighbour-count kernels of csrc/backbone2d3d.hip), in plain torch, written against the cited lines in our own words:

    kpconv_weighted     3D/models/blocks.py:288-393, the half of KPConv.forward before the product with the kernel weights: a shadow support at +1e6,
                        the influence of every kernel point on every neighbour ('constant' | 'linear' | 'gaussian'), 'closest' = only the nearest kernel
                        point of a neighbour (torch.argmin: first minimum), the sum over the neighbours, the division by the number of neighbours whose
                        feature sum is > 0 (at least 1)
    norm_block64        blocks.py:430-446 (InstanceNorm1d over the points: per column, biased variance, eps 1e-5, no affine) fused with LeakyReLU(0.1)
                        and the residual sum of blocks.py:650-660, in the four forms dr_norm_apply_f32 has
    max_pool64 / closest_pool64   blocks.py:56-87 with a zero shadow row; the maximum belongs to the FIRST maximal neighbour, stated with an explicit
                        first-occurrence mask so that autograd sends the gradient there whatever torch.max's own tie rule is
    knn_interpolate64   vision3d/ops/knn_interpolate.py:43-77 (k = None): weights mask / (d^2 + 1e-8), normalised by (sum + 1e-8)

Every function takes `dtype`: float64 is the reference; the same expression in float32 on the device is torch's own float32 result, whose distance
from float64 sets the bar of the GPU tests (tests/test_point_backbone_edges_gpu.py: 4 x that distance, exact where it is 0).  Any id outside
[0, Ns) is a shadow entry, as in the kernels (the fixtures of the other files only ever hold Ns itself).

The builders draw from diffreg_hip.synth's integer hash (no golden scene) and ASSERT, on the float64 side, the margins that keep every discrete
decision of the kernels (neighbour count, argmin, argmax, LeakyReLU's sign) away from a float32 tie -- or make the tie exact on purpose.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from diffreg_hip import synth

SLOPE = 0.1
EPS = 1e-5
SHADOW_KINDS = ("ns", "beyond", "neg", "mixed")          # the shadow id a list is padded with: Ns | Ns + 7 | -1 | all three in turn


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_dev(a, ref):
    """max |a - ref| / max |ref| of two tensors (float64 arithmetic); 0 / inf when the reference is all zero"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    num, den = (a - ref).abs().max().item(), ref.abs().max().item()
    if den == 0.0:
        return 0.0 if num == 0.0 else math.inf
    return num / den


# ------------------------------------------------------------------------------------------------------------------------------------------
# the operations
# ------------------------------------------------------------------------------------------------------------------------------------------
def _shadowed(idx, n):
    """ids outside [0, n) -> n (the appended shadow row)"""
    return torch.where((idx < 0) | (idx >= n), torch.full_like(idx, n), idx)


def kpconv_weighted(q, s, idx, x, kp, extent, influence="linear", aggregation="sum", normalise=True, dtype=torch.float64):
    """-> (weighted [Nq, K Cin] with weighted[q][k Cin + c] = sum_h w[q][h][k] x[idx[q][h]][c] (/ max(1, count_q) when `normalise`), counts int64 [Nq])
    x may require grad (dtype float64: the reference gradient; float32: torch's own)."""
    q, s, x, kp = q.to(dtype), s.to(dtype), x.to(dtype), kp.to(dtype)
    Ns = s.shape[0]
    idx = _shadowed(idx, Ns)
    s_pad = torch.cat((s, torch.full_like(s[:1], 1e6)), 0)                       # :288 the shadow support
    rel = s_pad[idx] - q[:, None, :]                                             # :291-294 [Nq, H, 3]
    d2 = ((rel[:, :, None, :] - kp) ** 2).sum(3)                                 # :304-308 [Nq, H, K]
    if influence == "constant":
        w = torch.ones_like(d2)
    elif influence == "linear":
        w = torch.clamp(1 - torch.sqrt(d2) / extent, min=0.0)
    elif influence == "gaussian":
        w = torch.exp(-d2 / (2 * (extent * 0.3) ** 2 + 1e-9))
    else:
        raise ValueError(influence)
    if aggregation == "closest":                                                 # :324-326
        w = w * F.one_hot(torch.argmin(d2, dim=2), d2.shape[2]).to(dtype)
    elif aggregation != "sum":
        raise ValueError(aggregation)
    nx = torch.cat((x, torch.zeros_like(x[:1])), 0)[idx]                         # :369-372 [Nq, H, Cin]
    wf = torch.matmul(w.transpose(1, 2), nx)                                     # :375 [Nq, K, Cin]
    counts = (nx.sum(-1) > 0).sum(-1)                                            # :390-391
    wf = wf.reshape(wf.shape[0], -1)
    if normalise:
        wf = wf / counts.clamp(min=1)[:, None]                                   # :392-393
    return wf, counts


NORM_FORMS = ("a", "a_noact", "ab_norm", "ab_id")


def xhat64(x, dtype=torch.float64):
    x = x.to(dtype)
    m = x.mean(0)
    v = ((x - m) ** 2).mean(0)                                                   # biased
    return (x - m) / torch.sqrt(v + EPS), m, 1.0 / torch.sqrt(v + EPS)


def norm_pre64(a, b, form, dtype=torch.float64):
    """the value the activation sees: xhat_a + [xhat_b | b | 0]"""
    pre = xhat64(a, dtype)[0]
    if form == "ab_norm":
        pre = pre + xhat64(b, dtype)[0]
    elif form == "ab_id":
        pre = pre + b.to(dtype)
    return pre


def norm_block64(a, b=None, form="a", activate=None, slope=SLOPE, dtype=torch.float64):
    """form 'a': act(xhat_a); 'a_noact': xhat_a; 'ab_norm': act(xhat_a + xhat_b); 'ab_id': act(xhat_a + b).  `activate` overrides the form's own
    activation (the C entry takes the two independently)."""
    act = (form != "a_noact") if activate is None else activate
    pre = norm_pre64(a, b, form, dtype)
    return F.leaky_relu(pre, slope) if act else pre


def norm_block_torch32(a, b=None, form="a", activate=None, slope=SLOPE):
    """torch's own float32 result of the same block: F.instance_norm, as the module the kernels replace runs it (one row: F.instance_norm refuses
    a single spatial element, so the written-out expression in float32 stands in)"""
    act = (form != "a_noact") if activate is None else activate
    if a.shape[0] == 1:
        return norm_block64(a, b, form, act, slope, dtype=torch.float32)
    inorm = lambda x: F.instance_norm(x.t().unsqueeze(0), eps=EPS).squeeze(0).t()
    pre = inorm(a)
    if form == "ab_norm":
        pre = pre + inorm(b)
    elif form == "ab_id":
        pre = pre + b
    return F.leaky_relu(pre, slope) if act else pre


def max_pool64(x, inds, dtype=torch.float64):
    x = x.to(dtype)
    vals = torch.cat((x, torch.zeros_like(x[:1])), 0)[_shadowed(inds, x.shape[0])]          # [n2, H, d]
    is_max = vals.detach() == vals.detach().max(1, keepdim=True)[0]
    first = is_max & (is_max.cumsum(1) == 1)                                     # the first maximal neighbour, one per (row, channel)
    return (vals * first.to(dtype)).sum(1)


def closest_pool64(x, inds, dtype=torch.float64):
    x = x.to(dtype)
    return torch.cat((x, torch.zeros_like(x[:1])), 0)[_shadowed(inds[:, 0], x.shape[0])]


def knn_interpolate64(q, s, x, inds, dtype=torch.float64):
    q, s, x = q.to(dtype), s.to(dtype), x.to(dtype)
    Ns = s.shape[0]
    idx = _shadowed(inds, Ns)
    s_pad = torch.cat((s, torch.zeros_like(s[:1])), 0)
    x_pad = torch.cat((x, torch.zeros_like(x[:1])), 0)
    d2 = ((q[:, None, :] - s_pad[idx]) ** 2).sum(-1)
    w = (idx != Ns).to(dtype) / (d2 + 1e-8)                                      # :72-74: shadow entries weigh 0
    w = w / (w.sum(1, keepdim=True) + 1e-8)
    return (x_pad[idx] * w[..., None]).sum(1)


# ------------------------------------------------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------------------------------------------------
def unit_points(seed, stream, n):
    """n float32 points, uniform in the unit box"""
    return synth.hash_uniform(seed, stream, (n, 3), 0.0, 1.0).astype(np.float32)


def shadow_ids(kind, Ns, shape, seed=0):
    """int64 array of shadow ids of one kind (or the three kinds in turn along the flattened array)"""
    n = int(np.prod(shape))
    if kind == "mixed":
        v = np.array([Ns, Ns + 7, -1], dtype=np.int64)[(np.arange(n) + seed) % 3]
    else:
        v = np.full(n, {"ns": Ns, "beyond": Ns + 7, "neg": -1}[kind], dtype=np.int64)
    return v.reshape(shape)


def radius_lists(q, s, radius, H, shadow="ns", punch=0.0, seed=0):
    """brute force in float64 on the CPU: per query the supports with d < radius, ascending (d^2, index), the first H of them, padded with shadow
    ids of the given kind; `punch` = the share of real entries that is then replaced by a shadow id where it stands (shadows inside a row)"""
    q64, s64 = q.astype(np.float64), s.astype(np.float64)
    Nq, Ns = len(q64), len(s64)
    d2 = ((q64[:, None, :] - s64[None, :, :]) ** 2).sum(2)
    assert Ns >= H
    order = np.argsort(d2, axis=1, kind="stable")[:, :H]
    inside = np.take_along_axis(d2, order, 1) < radius * radius
    if punch > 0:
        inside &= synth.hash_u01(seed, 4242, Nq * H).reshape(Nq, H) >= punch
    return np.where(inside, order, shadow_ids(shadow, Ns, (Nq, H), seed)).astype(np.int64)


def kernel_points(seed, K, radius, mirror=False):
    """the centre plus K - 1 points at 0.6 radius in hashed directions (float32).  mirror: point 2 = point 1 reflected in the plane x = 0, both
    closer to that plane than any other kernel point is to a neighbour standing on it at their height (kpconv_case places one there)"""
    v = synth.hash_normal(seed, 77, (max(K - 1, 1), 3))
    v = v / np.sqrt((v * v).sum(1, keepdims=True)) * (0.6 * radius)
    kp = np.concatenate([np.zeros((1, 3)), v], 0)[:K].astype(np.float32)
    if mirror:
        kp[1] = np.array([0.12, 0.45, 0.30], dtype=np.float32) * np.float32(radius)
        kp[2] = kp[1] * np.array([-1.0, 1.0, 1.0], dtype=np.float32)
    return kp


def signed_features(seed, Ns, Cin, negative_rows):
    """x [Ns, Cin] float32 whose row sums are amp_r sgn_r with amp in [0.6, 1.5]: entries (amp sgn + 2 (n - mean_c n)) / Cin, so single entries
    carry either sign (Cin > 1) while the sum that decides KPConv's neighbour count stays >= 0.5 from zero.  Asserted here in float64."""
    n = synth.hash_normal(seed, 5, (Ns, Cin))
    amp = synth.hash_uniform(seed, 6, (Ns,), 0.6, 1.5)
    sgn = np.where(negative_rows, -1.0, 1.0)
    x = ((amp * sgn)[:, None] + 2.0 * (n - n.mean(1, keepdims=True))) / Cin
    x = x.astype(np.float32)
    assert np.abs(x.astype(np.float64).sum(1)).min() >= 0.5
    return x


def kpconv_case(Cin, H, K, shadow="mixed", Nq=1029, Ns=500, seed=1, mirror=False):
    """one KPConv geometry: queries and supports in the unit box, radius lists (about 1.2 H supports expected inside the radius, so most rows are
    full and rows near the faces are padded; 8 % of the real entries replaced by shadow ids in place), rows Nq - 5 .. Nq - 1 all shadow, sign-mixed
    features: >= a quarter of the supports carry a negative sum, and every real neighbour of query 3 does (count 0).
    -> dict of torch CPU tensors q, s, idx, x, kp and extent, radius"""
    sd = seed * 1000 + Cin * 7 + H * 3 + K
    q, s = unit_points(sd, 1, Nq), unit_points(sd, 2, Ns)
    radius = min(0.45, (1.2 * H / (Ns * 4.0 / 3.0 * math.pi)) ** (1.0 / 3.0))
    extent = 0.5 * radius
    idx = radius_lists(q, s, radius, H, shadow, punch=0.08, seed=sd)
    idx[Nq - 5:] = shadow_ids(shadow, Ns, (5, H), sd)
    kp = kernel_points(sd, K, radius, mirror)
    tie = None
    if mirror:                                                                   # support 0 at the midpoint of kernel points 1 and 2 as seen from query 7
        s[0] = q[7] + np.array([0.0, kp[1, 1], kp[1, 2]], dtype=np.float32)
        assert s[0, 0] == q[7, 0]
        idx = radius_lists(q, s, radius, H, shadow, punch=0.08, seed=sd)
        idx[Nq - 5:] = shadow_ids(shadow, Ns, (5, H), sd)
        idx[7, 0] = 0
        idx[7, 1:][idx[7, 1:] == 0] = Ns
        tie = (7, 0)
    real = (idx >= 0) & (idx < Ns)
    neg = synth.hash_u01(sd, 9, Ns) < 0.35
    qneg = int(np.argmax(real.sum(1) - 1000 * (np.arange(Nq) == 7)))          # the first query with the longest list (not the tie's query)
    neg[idx[qneg][real[qneg]]] = True
    x = signed_features(sd, Ns, Cin, neg)
    # the margins, from the float64 side alone
    sums = x.astype(np.float64).sum(1)
    assert (sums < 0).mean() >= 0.25 and np.abs(sums).min() >= 0.5
    assert not real[Nq - 5:].any() and real[:Nq - 5].any(1).mean() > 0.5
    cnt = ((np.concatenate([sums, [0.0]])[np.where(real, idx, Ns)] > 0) & real).sum(1)
    assert real[qneg].any() and cnt[qneg] == 0, "every neighbour of this query carries a negative sum"
    assert cnt.max() >= 1 and (cnt < real.sum(1)).any()
    for kind in ((Ns, Ns + 7, -1) if shadow == "mixed" else ()):
        assert (idx == kind).any()
    return dict(q=T(q), s=T(s), idx=T(idx), x=T(x), kp=T(kp), extent=extent, radius=radius, tie=tie, counts=T(cnt), qneg=qneg)


def closest_margin(case):
    """-> (smallest gap between the two nearest kernel-point distances over every real (query, neighbour) pair other than the deliberate tie,
    in units of extent; the gap of the tie pair, or None).  K = 1 has no second distance: inf."""
    q, s, idx, kp = (case[k].double() if k != "idx" else case[k] for k in ("q", "s", "idx", "kp"))
    Ns = s.shape[0]
    real = (idx >= 0) & (idx < Ns)
    if kp.shape[0] < 2:
        return math.inf, None
    rel = s[idx.clamp(0, Ns - 1)] - q[:, None, :]
    d = torch.sqrt(((rel[:, :, None, :] - kp) ** 2).sum(3)).sort(2)[0]
    gap = (d[:, :, 1] - d[:, :, 0]) / case["extent"]
    tie_gap = None
    if case["tie"] is not None:
        tie_gap = gap[case["tie"]].item()
        real = real.clone()
        real[case["tie"]] = False
    return gap[real].min().item(), tie_gap


# the thinned cross product of test 1: every Cin and every (H, K) at least twice, every CPL instantiation under every (H, K)
KP_CIN = (1, 63, 64, 65, 128, 129, 256, 257, 512)
KP_HK = ((1, 15), (17, 15), (64, 16), (33, 1))
_A, _B, _C, _D = KP_HK
KPCONV_CASES = [(1, _A), (1, _C), (63, _B), (63, _D), (64, _A), (64, _C), (65, _B), (65, _D), (65, _A), (128, _B), (128, _C), (129, _A), (129, _D),
                (256, _B), (256, _C), (257, _A), (257, _D), (257, _C), (512, _B), (512, _C), (512, _D)]
KPCONV_CASES = [(cin, h, k, SHADOW_KINDS[(i + 3) % 4]) for i, (cin, (h, k)) in enumerate(KPCONV_CASES)]


def cpl_of(Cin):
    """the instantiation kpconv_gather_kernel<CPL> the launcher picks"""
    return 1 if Cin <= 64 else 2 if Cin <= 128 else 4 if Cin <= 256 else 8


def kpconv_id(c):
    return "cin%d-cpl%d-h%d-k%d-shadow_%s" % (c[0], cpl_of(c[0]), c[1], c[2], c[3])


MODE_CASES = [(i, a) for i in ("constant", "linear", "gaussian") for a in ("sum", "closest")]
MODE_SHAPE = dict(Cin=96, H=24, K=15, Nq=257, Ns=200, seed=5)      # seeds 2, 3, 4 leave a pair under the 1e-4 extent margin of 'closest'


def mode_case():
    return kpconv_case(MODE_SHAPE["Cin"], MODE_SHAPE["H"], MODE_SHAPE["K"], "mixed", MODE_SHAPE["Nq"], MODE_SHAPE["Ns"], MODE_SHAPE["seed"], mirror=True)


# ---- the normalisation block -----------------------------------------------------------------------------------------------------------
NORM_N = (1, 2, 255, 256, 257, 1027, 16385, 16447)
NORM_C = (1, 31, 32, 33, 96, 200)
NORM_CASES = [(1, 1), (1, 33), (2, 31), (2, 96), (255, 32), (255, 200), (256, 1), (256, 33), (257, 31), (257, 96), (1027, 32), (1027, 200),
              (1027, 33), (16385, 1), (16385, 31), (16447, 33)]
NORM_SPECIAL = (1027, 33)            # this case carries a constant column (0) and a column of mean 1e4, spread 1 (the last)
NORM_COMBOS = [("a", True), ("a", False), ("ab_norm", True), ("ab_norm", False), ("ab_id", True), ("ab_id", False)]


def slabs_of(N):
    """(R, rows_per) of col_stats / norm_backward"""
    R = min(64, (N + 255) // 256)
    return R, (N + R - 1) // R


def norm_id(c):
    return "n%d-R%d-c%d" % (c[0], slabs_of(c[0])[0], c[1])


def sign_margin(a, b, form):
    """per entry: how far the activation's argument must stay from 0 for float32 to see its sign as float64 does: 1e-5 + 16 float32 ulps of the
    column's largest |value| times rstd (the rounding of the float32 mean alone moves xhat by half an ulp of the mean times rstd), summed over the
    normalised operands.  An argument that is exact in float32 as well (xhat_a = 0 identically -- a constant column, N = 1, a value equal to a
    representable mean -- plus nothing, b itself, or an xhat_b that is 0 likewise) is exempt: both precisions see the same number."""
    xa, _, ra = xhat64(a)
    m = 1e-5 + 16 * 2.0 ** -24 * a.double().abs().max(0)[0] * ra
    exact = xa == 0
    if form == "ab_norm":
        xb, _, rb = xhat64(b)
        m = m + 16 * 2.0 ** -24 * b.double().abs().max(0)[0] * rb
        exact = exact & (xb == 0)
    return m.expand_as(xa), exact


def norm_case(N, C, seed=3):
    """a = 3 n + 1, b = n', G = n'' (float32, hashed).  The special case's column 0 is constant (2.5), its last column is 1e4 + n.  Then the entries
    whose activation argument is closer to 0 than sign_margin are moved away from it (a in form 'a', b in the forms with b: one value each,
    a few ulps), per form; the margin is asserted on the result.  -> dict(a_<form>, b_<form> for the three activated forms, G)"""
    sd = seed * 100000 + N * 31 + C
    a0 = (3.0 * synth.hash_normal(sd, 1, (N, C)) + 1.0).astype(np.float32)
    b0 = synth.hash_normal(sd, 2, (N, C)).astype(np.float32)
    G = synth.hash_normal(sd, 3, (N, C)).astype(np.float32)
    if (N, C) == NORM_SPECIAL:
        a0[:, 0] = 2.5
        a0[:, C - 1] = (1e4 + synth.hash_normal(sd, 4, (N,))).astype(np.float32)
    if N == 2:          # two rows normalise to +-1 / sqrt(1 + eps / var) whatever their values: xhat_a + xhat_b of opposite order is a difference of
        swap = (a0[0] - a0[1]) * (b0[0] - b0[1]) < 0          # two such numbers, which no move of one value decides; give b the order of a
        b0[:, swap] = b0[::-1, swap]
    out = dict(G=T(G))
    for form in ("a", "ab_norm", "ab_id"):
        a, b = T(a0.copy()), T(b0.copy())
        for _ in range(4):
            pre = norm_pre64(a, b, form)
            m, exact = sign_margin(a, b, form)
            bad = (pre.abs() < m) & ~exact
            if not bad.any():
                break
            t = a if form == "a" else b
            scale = 1.0 / xhat64(t)[2].expand_as(pre) if form != "ab_id" else torch.ones_like(pre)
            step = torch.where(pre >= 0, 1.0, -1.0) * 3.0 * m * scale
            t[bad] = (t.double() + step)[bad].float()
        pre = norm_pre64(a, b, form)
        m, exact = sign_margin(a, b, form)
        assert bool(((pre.abs() >= m) | exact).all()), (N, C, form)
        out["a_" + form], out["b_" + form] = a, b
    return out


def leaky_zero_case(N=258, C=33, seed=4):
    """a whose columns 0 .. 3 are built from pairs mu +- d (mu = 0.5, d a multiple of 2^-12: the float64 sum of the column is N mu exactly, so the mean
    is mu in both precisions) with rows 0, 1, 2 and N - 1 holding mu itself: xhat is exactly 0 there, in float32 as in float64.  b (form ab_id) is 0
    at those entries.  -> dict(a, b, G, zeros = bool mask of the 16 entries)"""
    assert N % 2 == 0
    sd = seed * 100000 + N * 31 + C
    a = (3.0 * synth.hash_normal(sd, 1, (N, C)) + 1.0).astype(np.float32)
    b = synth.hash_normal(sd, 2, (N, C)).astype(np.float32)
    G = synth.hash_normal(sd, 3, (N, C)).astype(np.float32)
    zeros = np.zeros((N, C), bool)
    rows0 = np.array([0, 1, 2, N - 1])
    rest = np.setdiff1d(np.arange(N), rows0)
    for c in range(4):
        d = (np.floor(synth.hash_uniform(sd, 10 + c, (len(rest) // 2,), 1.0, 8000.0)) * 2.0 ** -12).astype(np.float32)
        a[rest[0::2], c] = np.float32(0.5) + d
        a[rest[1::2], c] = np.float32(0.5) - d
        a[rows0, c] = 0.5
        zeros[rows0, c] = True
    b[zeros] = 0.0
    a, b = T(a), T(b)
    for form in ("a", "ab_id"):
        pre = norm_pre64(a, b, form)
        assert bool((pre[T(zeros)] == 0).all()) and int((pre == 0).sum()) == 16
        m, _ = sign_margin(a, b, form)
        # elsewhere the sign is decided: move b (ab_id) where needed; form 'a' is asserted as drawn
        bad = (pre.abs() < m) & ~T(zeros)
        if form == "ab_id" and bad.any():
            b[bad] = (b.double() + torch.where(pre >= 0, 1.0, -1.0) * 3.0 * m)[bad].float()
            pre = norm_pre64(a, b, form)
            bad = (pre.abs() < m) & ~T(zeros)
        assert not bad.any(), form
    return dict(a=a, b=b, G=T(G), zeros=T(zeros))


# ---- pools -------------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = ((1, 1, 1), (300, 17, 96), (257, 64, 65), (100, 5, 200))


def pool_id(c):
    return "n%d-h%d-d%d-ld%d" % (c[0], c[1], c[2], c[3])


POOL_CASES = [(n2, H, d, H + e) for (n2, H, d) in POOL_SHAPES for e in (0, 3)]
POOL_GRID = 2.0 ** -9


def pool_case(n2, H, d, ld, seed=5):
    """x [n1, d] on a grid of 2^-9 (two values are bit-equal or >= 1.9e-3 apart: every tie is exact), rows 0 .. n1/4 all negative; a copy of one row
    in another; inds [n2, ld] (columns H .. ld - 1 hold an id the kernel must not read: 0 with max-pool would win over the negative block) with ids
    from [0, n1) and the three shadow kinds, all-shadow rows, rows that see only the negative block (with and without a shadow), rows that list the
    two bit-equal rows in either order, rows with the same id twice.  -> dict(x, inds [n2, ld], n1, G [n2, d])"""
    sd = seed * 100000 + n2 * 131 + H * 17 + d
    n1 = max(2, min(600, 2 * n2 + 5))
    x = np.round(synth.hash_normal(sd, 1, (n1, d)) / POOL_GRID) * POOL_GRID + 0.0
    nneg = max(1, n1 // 4)
    x[:nneg] = -np.abs(x[:nneg]) - POOL_GRID
    twin_a, twin_b = n1 - 1, n1 - 2
    x[twin_b] = x[twin_a]
    x = x.astype(np.float32)
    assert np.array_equal(x.astype(np.float64) / POOL_GRID, np.round(x.astype(np.float64) / POOL_GRID)) and (x[:nneg] < 0).all()
    u = synth.hash_u01(sd, 2, n2 * ld).reshape(n2, ld)
    inds = np.floor(synth.hash_u01(sd, 3, n2 * ld).reshape(n2, ld) * n1).astype(np.int64)
    sh = shadow_ids("mixed", n1, (n2, ld), sd)
    inds = np.where(u < 0.2, sh, inds)
    r = lambda k: k % n2
    if n2 >= 8:
        inds[r(1), :H] = sh[r(1), :H]                                            # all shadow
        inds[r(2), :H] = np.arange(H) % nneg                                     # only negative rows: the maximum is negative
        inds[r(3), :H] = np.arange(H) % nneg                                     # negative rows and a shadow: the shadow's zero wins, no gradient
        inds[r(3), H - 1] = sh[r(3), 0]
        inds[r(4), :H], inds[r(5), :H] = sh[r(4), :H], sh[r(5), :H]
        inds[r(4), 0], inds[r(5), 0] = twin_a, twin_b                            # the bit-equal rows in either order, shadows after them
        if H > 1:
            inds[r(4), 1], inds[r(5), 1] = twin_b, twin_a
            inds[r(6), 1] = inds[r(6), 0] = nneg + (n1 - nneg) // 2             # the same id twice
        inds[n2 - 1, :H] = sh[n2 - 1, :H]
    else:
        inds[0, 0] = n1 - 1
    inds[:, H:] = nneg                                                           # beyond H: a real, non-negative-block id that must stay unread
    G = synth.hash_normal(sd, 4, (n2, d)).astype(np.float32)
    return dict(x=T(x), inds=T(inds), n1=n1, G=T(G))


# ---- kNN interpolation -----------------------------------------------------------------------------------------------------------------------
KNN_C = (1, 63, 64, 65, 256)
KNN_H = (1, 3, 64)
KNN_CASES = [(C, H) for C in KNN_C for H in KNN_H]


def knn_id(c):
    return "c%d-h%d" % c


def knn_case(C, H, Nq=1029, Ns=300, seed=6):
    """queries / supports in the unit box, radius lists with shadows punched into the rows (inside and at the end), the last three rows all shadow,
    queries 10 .. 19 moved onto a support that stands first in their list (d = 0 exactly), x and the upstream gradient hashed normals"""
    sd = seed * 100000 + C * 131 + H
    q, s = unit_points(sd, 1, Nq), unit_points(sd, 2, Ns)
    radius = min(0.6, (1.5 * H / (Ns * 4.0 / 3.0 * math.pi)) ** (1.0 / 3.0) + 0.05)
    for i in range(10, 20):
        q[i] = s[(7 * i) % Ns]
    idx = radius_lists(q, s, radius, H, "mixed", punch=0.1, seed=sd)
    for i in range(10, 20):
        idx[i, 0] = (7 * i) % Ns
        assert np.array_equal(q[i], s[idx[i, 0]])
    idx[Nq - 3:] = shadow_ids("mixed", Ns, (3, H), sd)
    real = (idx >= 0) & (idx < Ns)
    assert real.any(1).mean() > 0.5
    if H >= 3:
        assert (~real[:, :-1] & real[:, 1:]).any() and (real[:, :-1] & ~real[:, 1:]).any(), "shadows inside and at the end of a row"
    x = synth.hash_normal(sd, 3, (Ns, C)).astype(np.float32)
    G = synth.hash_normal(sd, 4, (Nq, C)).astype(np.float32)
    return dict(q=T(q), s=T(s), idx=T(idx), x=T(x), G=T(G))
