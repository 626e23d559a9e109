"""Digests of what the two denoise loops compute and launch, for A/B runs of two builds whose device work must be identical (a host-side
refactor of loop.hip / loop2d3d.hip): one JSON object per case with the sha256 of every returned tensor, the match lists, the launch counts
and work per kernel family (lib.prof_collect) and the workspace / prepack sizes.  Run it on each build on the same GPU and compare the lines:
    python tools/loop_digest.py --out a.jsonl        (in each tree)
    python tools/loop_digest.py --compare a.jsonl b.jsonl   (verdict + the sha256 of every case's line in either file)"""
import argparse, ctypes, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd")); sys.path.insert(0, ROOT)

DEV, STEPS, MC = "cuda:0", 2, 200.0
LAYERS = (1, 2, 3, 6)
SHAPES_3D = ((2, 96, 160, False), (2, 128, 256, True), (1, 128, 128, False))       # P, N, M, masked + ragged (second pair's extents: 96 x 160)
SHAPES_2D3D = ((2, 96, 160), (1, 128, 256))
TENSORS = ("conf_matrix_pred", "x_final", "x0", "R_forwd", "t_forwd", "cond")


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def profiled(lib, fn):
    lib.prof_collect()                        # (drop what earlier calls recorded)
    lib.prof_enable(True)
    try:
        out = fn()
        prof = lib.prof_collect()
    finally:
        lib.prof_enable(False)
    return out, {k: [v[0], v[2]] for k, v in prof.items()}


def cases():
    import numpy as np
    import torch
    from diffreg_hip import lib, synth
    from diffreg_hip.engine import DenoiseEngine, DenoiseEngine2D3D
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    for variant in ("3dmatch", "4dmatch"):
        v = synth.VARIANTS[variant]
        W = {k: T(a) for k, a in synth.make_weights(v["C"], seed=7, head_gain=3.0).items()}          # the "soft" head of the tests
        for P, N, M, ragged in SHAPES_3D:
            seeds = [31 + N + i for i in range(P)]
            prs = [synth.make_pair(N, M, v["C"], seed=s) for s in seeds]
            a = [torch.stack([T(p[k]) for p in prs]).to(DEV) for k in ("src_feats", "tgt_feats", "s_pcd", "t_pcd", "x_T")]
            noise = torch.from_numpy(np.stack([synth.step_noise(N, M, s, STEPS) for s in seeds], 1)).to(DEV) if variant == "4dmatch" else None
            sm = tm = None
            if ragged:
                sm = torch.stack([torch.arange(N) < n for n in (N, 96)[:P]]).to(DEV)
                tm = torch.stack([torch.arange(M) < m for m in (M, 160)[:P]]).to(DEV)
            for nl in LAYERS:
                for planes in (True, False):
                    eng = DenoiseEngine(W, variant=variant, C=v["C"], H=v["H"], voxel=v["voxel"], origin=v["origin"], steps=STEPS, sk_iters=v["skh_iters"],
                                        sample_rate=v["sample_rate"], max_condition_num=MC, n_layers=nl, device=DEV, planes=planes)
                    out, prof = profiled(lib, lambda: eng.run(*a, sm, tm, noise=noise, trace=True, graph=False, ragged=ragged))
                    out["_status"].check()
                    rec = dict(case="%s P%d N%d M%d%s L%d %s" % (variant, P, N, M, " ragged" if ragged else "", nl, "planes" if planes else "f32"),
                               sha={k: sha(out[k]) for k in TENSORS}, launches=prof,
                               workspace_bytes=lib.raw().dr_denoise_loop_workspace_bytes(ctypes.byref(eng.cfg), P, N, M),
                               prepack_bytes=lib.raw().dr_loop_prepack_bytes(ctypes.byref(eng.cfg)))
                    if "match_count" in out:
                        rec["matches"] = [m.cpu().tolist() for m in eng.match_list(out)]
                    yield rec
                    if nl == 6 and (P, N) == (2, 96):      # one denoiser + matching-head evaluation (dr_denoiser_match_f32)
                        (so, to, conf), prof = profiled(lib, lambda: eng.denoise_match(*a[:4]))
                        yield dict(case="%s denoise_match %s" % (variant, "planes" if planes else "f32"),
                                   sha=dict(src_out=sha(so), tgt_out=sha(to), conf=sha(conf)), launches=prof)
    Wn = synth.make_weights_2d3d(seed=9, head_gain=16.0)
    W = {k: T(a) for k, a in Wn.items()}
    for P, N, M in SHAPES_2D3D:
        prs = [synth.make_pair_2d3d(N, M, 41 + i, weights=Wn) for i in range(P)]
        d = lambda k: torch.stack([T(p[k]) for p in prs]).to(DEV)
        masks = tuple(torch.stack([torch.arange(L) < L - c - 3 * i for i in range(P)]).to(DEV) for L, c in ((N, 6), (M, 10), (M, 19)))
        for nl in LAYERS:
            for planes in (True, False):
                eng = DenoiseEngine2D3D(W, steps=STEPS, max_condition_num=MC, n_layers=nl, device=DEV, planes=planes)
                out, prof = profiled(lib, lambda: eng.run(d("img_feats"), d("img_dino"), d("img_pixels"), d("pcd_feats"), d("s_pcd"), d("t_pcd_da"),
                                                          d("x_T"), masks, trace=True))
                cnt = out["match_count"].cpu().tolist()
                out["_status"].check()
                cfg = eng._cfg(STEPS)
                yield dict(case="2d3d P%d N%d M%d masked L%d %s" % (P, N, M, nl, "planes" if planes else "f32"),
                           sha={k: sha(out[k]) for k in TENSORS}, launches=prof,
                           matches=[out["matches_padded"][p, :cnt[p]].cpu().tolist() for p in range(P)],
                           workspace_bytes=lib.raw().dr_denoise_loop_2d3d_workspace_bytes(ctypes.byref(cfg), P, N, M),
                           prepack_bytes=lib.raw().dr_loop2d3d_prepack_bytes(ctypes.byref(cfg)))
                if nl == 6 and P == 2:                     # component mode: one fusion + matching evaluation (steps = 0)
                    (fi, fp, c0), prof = profiled(lib, lambda: eng.fuse_and_match(d("img_feats"), d("img_dino"), d("img_pixels"), d("pcd_feats"),
                                                                                  d("s_pcd"), masks))
                    yield dict(case="2d3d fuse_and_match %s" % ("planes" if planes else "f32"), sha=dict(img=sha(fi), pcd=sha(fp), conf=sha(c0)),
                               launches=prof)


def compare(fa, fb):
    """-> the verdict, with the sha256 of each case's whole output line in either file (the compact form of the two outputs that is kept on record)"""
    a, b = ({json.loads(l)["case"]: hashlib.sha256(l.strip().encode()).hexdigest() for l in open(f)} for f in (fa, fb))
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print(json.dumps(dict(cases=len(a), equal=not bad, differing=bad, line_sha256={k: [a.get(k), b.get(k)] for k in sorted(set(a) | set(b))}), indent=1))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the lines to this file")
    ap.add_argument("--compare", nargs=2, metavar="FILE")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    f = open(args.out, "w") if args.out else None
    for rec in cases():
        line = json.dumps(rec, sort_keys=True)
        print(line, flush=True)
        if f:
            f.write(line + "\n"); f.flush()
