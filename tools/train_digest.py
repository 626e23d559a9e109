"""Digests of what the training layers compute and launch, for A/B runs of two builds whose device work must be identical (a host-side refactor
of autograd.py / train_layer.hip / train_fusion.hip / circle_loss.hip): one JSON object per case with the sha256 of every output tensor and every
gradient and the launch counts per kernel family (lib.prof_collect).  Run it on each build on the same GPU -- twice on the older one -- and compare:
    python tools/train_digest.py --out a.jsonl [--tensors a_dir]        (in each tree; --tensors keeps every tensor, one .npz per case)
    python tools/train_digest.py --compare a.jsonl b.jsonl [--again a2.jsonl --tensors a_dir b_dir a2_dir]
--compare prints the verdict and the sha256 of every case's line in either file.  A case whose line differs between the older build's own two runs
(a.jsonl, a2.jsonl) is not bit-stable: there the newer build's tensors may differ from a's by no more than a2's do (maximum absolute difference,
tensor by tensor), and its launch counts must still be equal.
A case the library refuses (a head width that is no multiple of 4) is recorded with the error it raises: both builds must refuse it alike."""
import argparse, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd")); sys.path.insert(0, ROOT)

DEV = "cuda:0"
# (B, L, S, C, H); y_is_x: the call's two inputs are one tensor (S = L)
FUSED_LAYER = (((1, 64, 48, 132, 4), True, False), ((1, 64, 48, 132, 3), True, False), ((2, 101, 75, 432, 4), True, False),
               ((2, 64, 64, 256, 4), False, True), ((3, 7, 5, 8, 2), True, False))          # shape, masked, y_is_x
PER_OP_LAYER = ((1, 64, 48, 132, 4), (1, 64, 48, 132, 3))
HEAD = (1, 64, 48, 132)                                                                      # B, N, M, C
FUSION_LAYER = ((2, 64, 96, 256, 4), (3, 7, 5, 8, 2))
CIRCLE = ((48, 32, 132), (97, 130, 256))                                                     # M, N, C


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def cases():
    import torch
    from diffreg_hip import autograd as dag, lib
    gen = torch.Generator().manual_seed(20)
    rnd = lambda *shape, s=1.0: (torch.randn(*shape, generator=gen) * s).to(DEV)

    def tables(rows, C):
        a = rnd(rows, C // 2, s=3.0)
        return a.cos().contiguous(), a.sin().contiguous()

    def masks(B, L, S):
        ar = lambda n, cut: (torch.arange(n)[None] < torch.tensor([[n - cut * (b + 1)] for b in range(B)])).to(DEV)
        return ar(L, 1), ar(S, 1)

    class Layer(torch.nn.Module):              # the attributes geometry_attention_layer reads of a models.transformero.GeometryAttentionLayer
        def __init__(self, C, H, pe_type):
            super().__init__()
            lin = lambda i, o: torch.nn.Linear(i, o, bias=False)
            self.q_proj, self.k_proj, self.v_proj, self.merge = lin(C, C), lin(C, C), lin(C, C), lin(C, C)
            self.mlp = torch.nn.Sequential(lin(2 * C, 2 * C), torch.nn.ReLU(), lin(2 * C, C))
            self.norm1, self.norm2 = torch.nn.LayerNorm(C), torch.nn.LayerNorm(C)
            self.nhead, self.pe_type = H, pe_type
            with torch.no_grad():
                for p in self.parameters():
                    p.copy_(torch.randn(p.shape, generator=gen) * (0.3 if p.dim() == 1 else p.shape[1] ** -0.5) + (1.0 if p.dim() == 1 else 0.0))

    class Head(torch.nn.Module):               # the attributes matching_head_form reads of a models.matching.Matching
        def __init__(self, C, entangled, match_type):
            super().__init__()
            self.src_proj = torch.nn.Linear(C, C, bias=False)
            self.bin_score = torch.nn.Parameter(torch.tensor(1.0))
            self.entangled, self.match_type, self.skh_iters, self.temperature = entangled, match_type, 3, 0.1
            with torch.no_grad():
                self.src_proj.weight.copy_(torch.randn(C, C, generator=gen) * 3.0 * C ** -0.5)

    def run(name, fn):
        """fn() -> {tensor name: tensor}; the case's record, or the library's refusal"""
        lib.prof_collect()                      # (drop what earlier calls recorded)
        lib.prof_enable(True)
        try:
            out = fn()
            prof = lib.prof_collect()
        except RuntimeError as e:
            return dict(case=name, error=str(e)), {}
        finally:
            lib.prof_enable(False)
        return dict(case=name, sha={k: sha(v) for k, v in out.items()}, launches={k: v[0] for k, v in prof.items() if v[0]}), out

    def through_autograd(call, inputs, module):
        """call() -> the differentiable output; -> the output, the gradients of `inputs` and of the module's parameters under a fixed weighting"""
        out = call()
        (out * rnd(*out.shape)).sum().backward()
        res = dict(out=out.detach())
        res.update({"grad_" + k: t.grad for k, t in inputs.items()})
        res.update({"grad_" + k: p.grad for k, p in module.named_parameters() if p.grad is not None})
        return res

    # ---- GeometryAttentionLayer, the two fused library calls
    for (B, L, S, C, H), masked, y_is_x in FUSED_LAYER:
        layer = Layer(C, H, "rotary").to(DEV)
        wts = [p.detach().contiguous() for p in dag._layer_params(layer)]
        x = rnd(B, L, C, s=0.5)
        y = x if y_is_x else rnd(B, S, C, s=0.5)
        tx = tables(B * L, C)
        ty = tx if y_is_x else tables(B * S, C)
        xm, ym = masks(B, L, S) if masked else (None, None)
        go = rnd(B, L, C)

        def fused():
            out, saved = lib.attention_layer_train_forward(wts, C, H, x, y, *tx, *ty, xm, ym)
            gx, gy, gw = lib.attention_layer_backward(wts, C, H, x, y, *tx, *ty, xm, ym, saved, go)
            return dict(out=out, grad_x=gx, grad_y=gy, **{"grad_" + k: g for k, g in zip(lib._LAYER_KEYS, gw)})
        yield run("fused layer B%d L%d S%d C%d H%d%s%s" % (B, L, S, C, H, " masked" if masked else "", " y_is_x" if y_is_x else ""), fused)

    # ---- GeometryAttentionLayer, one library call per kernel: the shipped form with fused = False, the sinusoidal and the no-code form
    for B, L, S, C, H in PER_OP_LAYER:
        for form in ("rotary per-op", "sinusoidal", "no code"):
            for masked in (True, False):
                layer = Layer(C, H, "sinusoidal" if form == "sinusoidal" else "rotary").to(DEV)
                x, y = rnd(B, L, C, s=0.5).requires_grad_(True), rnd(B, S, C, s=0.5).requires_grad_(True)
                xm, ym = masks(B, L, S) if masked else (None, None)
                if form == "rotary per-op":
                    px, py = tables(B * L, C), tables(B * S, C)
                    call = lambda: dag.geometry_attention_layer(layer, x, y, px, py, xm, ym)
                else:
                    px, py = (rnd(B, L, C), rnd(B, S, C)) if form == "sinusoidal" else (None, None)
                    call = lambda: dag.geometry_attention_layer_form(layer, x, y, px, py, xm, ym)

                def per_op():
                    before = dag._GeometryAttentionLayer.fused
                    dag._GeometryAttentionLayer.fused = False
                    try:
                        return through_autograd(call, dict(x=x, y=y), layer)
                    finally:
                        dag._GeometryAttentionLayer.fused = before
                yield run("layer %s B%d L%d S%d C%d H%d%s" % (form, B, L, S, C, H, " masked" if masked else ""), per_op)

    # ---- the matching head: the shipped form and the three others
    B, N, M, C = HEAD
    for form in ("rotary sinkhorn", "none", "add", "rotary dual_softmax"):
        for masked in (True, False):
            head = Head(C, form == "none", "dual_softmax" if form.endswith("dual_softmax") else "sinkhorn").to(DEV)
            s, t = rnd(B, N, C).requires_grad_(True), rnd(B, M, C).requires_grad_(True)
            sm, tm = masks(B, N, M) if masked else (None, None)
            if form == "rotary sinkhorn":
                ps, pt = tables(B * N, C), tables(B * M, C)
                call = lambda: dag.matching_head(s, t, head.src_proj.weight, head.bin_score, ps, pt, sm, tm, 3)
            else:
                pe_type = "sinusoidal" if form == "add" else "rotary"
                ps, pt = (rnd(B, N, C), rnd(B, M, C)) if form == "add" else (tables(B * N, C), tables(B * M, C))
                call = lambda: dag.matching_head_form(head, s, t, ps, pt, sm, tm, pe_type)
            yield run("head %s N%d M%d C%d%s" % (form, N, M, C, " masked" if masked else ""), lambda: through_autograd(call, dict(src=s, tgt=t), head))

    # ---- the 2D-3D fusion layer, the two library calls
    for B, L, S, C, H in FUSION_LAYER:
        shapes = [(C, C), (C,)] * 4 + [(C,), (C,), (2 * C, C), (2 * C,), (C, 2 * C), (C,), (C,), (C,)]
        wts = [rnd(*sh, s=0.3 if len(sh) == 1 else sh[1] ** -0.5) + (1.0 if k.endswith("norm.weight") else 0.0) for k, sh in zip(lib.FUSION_LAYER_KEYS, shapes)]
        for kind in ("key mask", "no mask", "self"):
            x = rnd(B, L, C, s=0.5)
            y = x if kind == "self" else rnd(B, S, C, s=0.5)
            ym = masks(B, L, S)[1] if kind == "key mask" else None
            go = rnd(B, L, C)

            def fusion():
                out, saved = lib.fusion_layer_train_forward(wts, C, H, x, y, ym)
                gx, gy, gw = lib.fusion_layer_backward(wts, C, H, x, y, ym, saved, go)
                return dict(out=out, grad_x=gx, grad_y=gy, **{"grad_" + k: g for k, g in zip(lib.FUSION_LAYER_KEYS, gw)})
            yield run("fusion layer %s B%d L%d S%d C%d H%d" % (kind, B, L, y.shape[1], C, H), fusion)

    # ---- the circle loss
    params = lib.circle_params(0.1, 1.4, 0.1, 1.4, 40.0, 0.3, 0.2)          # margins, optima, log scale; positive: min overlap > 0.3, negative: max overlap < 0.2
    for M, N, C in CIRCLE:
        img, pcd = (torch.nn.functional.normalize(rnd(n, C), dim=1) for n in (M, N))
        K = 3 * M
        pairs = torch.randperm(M * N, generator=gen)[:K]
        ii, jj = (pairs // N).to(DEV), (pairs % N).to(DEV)
        omin = (torch.rand(K, generator=gen) * 0.6).to(DEV)
        omax = (omin + 0.2).clamp(max=1.0)
        gl = torch.tensor(0.7, device=DEV)

        def circle():
            loss = lib.circle_loss(img, pcd, ii, jj, omin, omax, params)
            loss_b, gi, gp = lib.circle_loss_backward(img, pcd, ii, jj, omin, omax, params, gl)
            return dict(loss=loss, loss_backward=loss_b, grad_img=gi, grad_pcd=gp)
        yield run("circle loss M%d N%d C%d" % (M, N, C), circle)


def compare(fa, fb, fa2=None, tensors=None):
    """-> the verdict, with the sha256 of each case's whole output line in every file (the compact form of the outputs that is kept on record)"""
    import numpy as np
    lines = [{json.loads(l)["case"]: l.strip() for l in open(f)} for f in (fa, fb) + ((fa2,) if fa2 else ())]
    a, b = lines[0], lines[1]
    a2 = lines[2] if fa2 else a
    names = sorted(set(a) | set(b) | set(a2))
    unstable = sorted(k for k in names if a.get(k) != a2.get(k))
    bad, noise = [], {}
    for k in names:
        if a.get(k) == b.get(k):
            continue
        if k not in unstable or not tensors or k not in b or json.loads(a[k]).get("launches") != json.loads(b[k]).get("launches"):
            bad.append(k)
            continue
        ta, tb, ta2 = (np.load(os.path.join(d, k.replace(" ", "_") + ".npz")) for d in tensors)
        d_new = {n: float(np.abs(tb[n] - ta[n]).max()) for n in ta.files}
        d_own = {n: float(np.abs(ta2[n] - ta[n]).max()) for n in ta.files}
        noise[k] = dict(new_vs_old=d_new, old_vs_old=d_own)
        if any(not d_new[n] <= d_own[n] for n in d_new):
            bad.append(k)
    h = lambda l: hashlib.sha256(l.encode()).hexdigest() if l is not None else None
    print(json.dumps(dict(cases=len(names), equal=not bad, differing=bad, not_bit_stable=unstable, numeric=noise,
                          line_sha256={k: [h(x.get(k)) for x in lines] for k in names}), indent=1))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the lines to this file")
    ap.add_argument("--tensors", nargs="+", metavar="DIR", help="with --out: keep every case's tensors here; with --compare: the three runs' directories")
    ap.add_argument("--compare", nargs=2, metavar="FILE")
    ap.add_argument("--again", metavar="FILE", help="with --compare: the second run of the first file's build")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare, args.again, args.tensors))
    f = open(args.out, "w") if args.out else None
    if args.tensors:
        os.makedirs(args.tensors[0], exist_ok=True)
    for rec, out in cases():
        line = json.dumps(rec, sort_keys=True)
        print(line, flush=True)
        if f:
            f.write(line + "\n"); f.flush()
        if args.tensors and out:
            import numpy as np
            np.savez(os.path.join(args.tensors[0], rec["case"].replace(" ", "_") + ".npz"), **{k: v.detach().cpu().numpy() for k, v in out.items()})
