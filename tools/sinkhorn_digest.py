"""Digests of what dr_sinkhorn_f32 / _f64 / _f16 compute, launch and ask for, for A/B runs of two builds whose device work must be identical
(a host-side refactor of sinkhorn.hip): one JSON object per case with the sha256 of the output, the return code, the PK_SINKHORN record count
and work (lib.prof_collect) and dr_sinkhorn_workspace_bytes for the case's element size and flags.  The cases are the smallest shapes at which
each decision of the launch plan can go wrong (form, rows per wave, float4 groups, columns per lane, type pair, vector access, refusals); which
kernel each one reaches shows in a kernel trace of the run (the persistent and per-tile kernels give the same bits by design).  Run it on each
build on the same GPU and compare the lines:
    python tools/sinkhorn_digest.py --out a.jsonl        (in each tree)
    python tools/sinkhorn_digest.py --compare a.jsonl b.jsonl   (verdict + the sha256 of every case's line in either file)"""
import argparse, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd")); sys.path.insert(0, ROOT)

DEV, ITERS = "cuda:0", 3
F32, F64, F64_32, F64_S, F16 = ("f32", {}), ("f64", {}), ("f64", dict(out_f32=True)), ("f64", dict(strict=True)), ("f16", {})


def C(name, B, N, M, types=(F32,), **kw):
    return [dict(name="%s %s%s%s %dx%dx%d" % (name, dt, "->f32" if tkw.get("out_f32") else "", " strict" if tkw.get("strict") else "", B, N, M),
                 dt=dt, B=B, N=N, M=M, **tkw, **kw) for dt, tkw in types]


def case_list(n_cu=256):
    """keywords: masked / minshift / ragged / log / out_f32 / strict (flags), iters, env (DR_* knobs behind dr_debug_enable_env), ws_delta (bytes
    added to the queried workspace size that the call is told about), null_out"""
    reg = (F32, F64_32, F64)
    L = []
    for N, M in ((96, 80), (130, 60), (64, 250), (255, 253), (128, 128), (256, 256)):     # register forms: the three tile classes, scalar access, plain tiles
        L += C("reg", 2, N, M, reg)
    for N, M in ((5, 7), (128, 128), (256, 256)):
        L += C("reg masked", 2, N, M, reg, masked=True)
    L += C("reg minshift masked", 3, 256, 256, reg, masked=True, minshift=True)
    L += C("reg ragged", 2, 96, 80, reg, masked=True, ragged=True)
    L += C("reg nt persistent", 512, 256, 256) + C("reg nt persistent", 513, 256, 256)
    L += C("reg nt per-tile", 512, 256, 256, env=dict(DR_SK_PERSIST_GRID="0"))
    L += C("reg no nt", 512, 256, 256, (F64_32,)) + C("reg below nt", 511, 256, 256) + C("reg nt", 2048, 128, 128) + C("reg below nt", 2047, 128, 128)
    L += C("coop 1 row", 2, 300, 400, reg)
    for M in (512, 768, 769):                                                              # two rows per wave up to 768 columns, then the batch form
        # (769 with float scores only: with double scores the 4-group batch kernel's scalar-access path does not repeat its own bits from run to
        #  run on the build before the launch plan either, and once ended in a memory fault -- profiles/sk_plan_ab.json; the cause is open, the batch
        #  form's launcher was therefore left as it was, and the case stays out until the kernel is understood)
        L += C("coop 2 rows", 8, 512, M, reg if M != 769 else (F32,))
    L += C("coop off", 2, 300, 400, env=dict(DR_SK_COOP="0")) + C("coop 1 row only", 8, 512, 512, env=dict(DR_SK_COOP="2"))
    L += C("batch 4 groups", 16, 512, 800, reg) + C("batch 8 groups", 16, 512, 1100, reg) + C("batch 8 groups", 8, 1024, 1280)
    L += C("batch off", 16, 512, 800, env=dict(DR_SK_BATCH="0"))
    L += C("batch one above the CUs", n_cu + 1, 32, 1100)                                  # B G = CU count + 1 (one workgroup per tile): the grid form
    for N, M in ((512, 512), (300, 1000), (300, 1100), (300, 1001)):                       # grid: 8 / 16 / 32 columns per lane, scalar access
        L += C("grid", 40, N, M, reg)
    L += C("grid log", 1, 40, 300, (F32, F64_S), log=True) + C("grid", 1, 300, 400, (F64_S, ("f64", dict(strict=True, out_f32=True))))
    L += C("grid 64 workgroups", 40, 512, 512, env=dict(DR_SK_GRID_WGS="64", DR_SK_GRID_CAP="1"))
    L += C("stream minshift", 2, 300, 400, (F32, F64, F64_S), minshift=True, masked=True) + C("stream wide", 2, 24, 2100, (F32, F64_S))
    for N, M in ((256, 256), (128, 128), (5, 7)):
        L += C("f16", 3, N, M, (F16,))
    L += C("f16 masked", 2, 96, 80, (F16,), masked=True) + C("f16 refused", 1, 300, 300, (F16,))
    L += C("refused iters 0", 2, 96, 80, iters=0) + C("refused null out", 2, 96, 80, null_out=True) + C("empty batch", 0, 96, 80)
    L += C("refused one byte short grid", 40, 512, 512, ws_delta=-1) + C("refused one byte short stream", 2, 24, 2100, ws_delta=-1)
    L += C("refused one byte short coop", 2, 300, 400, ws_delta=-1) + C("refused one byte short batch", 16, 512, 800, ws_delta=-1)
    L += C("refused iters 17 grid", 40, 301, 1000, iters=17)        # 40 x 301 x 1000: the 17th iteration's slot crosses the tile's 16-byte rounding
    L += C("iters 17 with room", 40, 301, 1000, iters=17, ws_delta=40 * 16)
    return L


def run(lib, torch, c):
    B, N, M, dt = c["B"], c["N"], c["M"], c["dt"]
    tdt = dict(f32=torch.float32, f64=torch.float64, f16=torch.float16)[dt]
    g = torch.Generator().manual_seed(1000 * N + M + B)
    x = (torch.randn(max(B, 1), N, M, generator=g) * 3 + (1.5 if c.get("minshift") else 0)).to(tdt).to(DEV)
    sm = tm = None
    if c.get("masked"):
        b = torch.arange(max(B, 1))[:, None]
        sm = lib.mask_u8((torch.arange(N)[None] < (N - N // 8 - 1 - b).clamp_min(1)).to(DEV))
        tm = lib.mask_u8((torch.arange(M)[None] < (M - M // 8 - 2 - 2 * b).clamp_min(1)).to(DEV))
    flags = (lib.SK_OUT_LOG if c.get("log") else 0) | (lib.SK_MINSHIFT if c.get("minshift") else 0) | (lib.SK_APPLY_MASK if c.get("masked") else 0) | \
            (lib.SK_OUT_F32 if c.get("out_f32") else 0) | (lib.SK_STRICT if c.get("strict") else 0) | (lib.SK_RAGGED if c.get("ragged") else 0)
    odt = tdt if dt != "f64" or not c.get("out_f32") else torch.float32
    out = torch.zeros((max(B, 1), N + 1, M + 1) if c.get("log") else (max(B, 1), N, M), dtype=odt, device=DEV)
    bs = torch.tensor([0.8], device=DEV)
    r, env = lib.raw(), c.get("env", {})
    if env:
        r.dr_debug_enable_env(1); os.environ.update(env)
    try:
        wsb = r.dr_sinkhorn_workspace_bytes(B, N, M, x.element_size(), flags)
        ws = torch.empty(max(wsb + max(c.get("ws_delta", 0), 0), 1), dtype=torch.uint8, device=DEV)
        lib.prof_collect(); lib.prof_enable(True)
        a = (B, N, M, lib.ptr(x), lib.ptr(sm), lib.ptr(tm), lib.ptr(bs), c.get("iters", ITERS), flags, None if c.get("null_out") else lib.ptr(out))
        if dt == "f16":
            rc = r.dr_sinkhorn_f16(*a, lib.stream_of(x))
        else:
            rc = (r.dr_sinkhorn_f64 if dt == "f64" else r.dr_sinkhorn_f32)(*a, lib.ptr(ws) if wsb else None, wsb + c.get("ws_delta", 0), lib.stream_of(x))
        prof = lib.prof_collect()["sinkhorn"]
    finally:
        lib.prof_enable(False)
        for k in env:
            os.environ.pop(k)
        if env:
            r.dr_debug_enable_env(1 if os.environ.get("DR_DIAGNOSTICS") == "1" else 0)
    lib.device_status(DEV)                       # raises on a co-resident time-out
    return dict(case=c["name"], rc=rc, sha256=hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest(), launches=[prof[0], prof[2]], workspace_bytes=wsb)


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
    import torch
    from diffreg_hip import lib
    lib.ensure_init()
    f = open(args.out, "w") if args.out else None
    for c in case_list(torch.cuda.get_device_properties(0).multi_processor_count):
        line = json.dumps(run(lib, torch, c), sort_keys=True)
        print(line, flush=True)
        if f:
            f.write(line + "\n"); f.flush()
