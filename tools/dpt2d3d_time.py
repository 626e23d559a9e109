"""Time the Depth-Anything DPT head's forward on one GPU:

    python tools/dpt2d3d_time.py [--out FILE.json]

Geometry: the model's (EXP/model.py:176-190: 476 x 630 -> a 34 x 45 patch grid of width 1 024), features 256, out_channels [256, 512, 1024, 1024],
random weights (tests/dpt2d3d_ref.draw_weights).  Method of DESIGN 5f-5p: 5 warm-up runs, then 30 runs alternating the two sides, each between
two device synchronisations; median [p10-p90] in milliseconds.  The baseline is the reference-shaped module (tests/dpt2d3d_ref.DPTHead: nothing is
read from the reference) in plain PyTorch float32 on the same GPU, under torch.no_grad().  Every item runs in a child process of its own under
its own time limit; the first one that fails ends the run.  Items:
 head       DeviceDPTHead.forward against the module's own forward, and the multiply-adds of the head counted from the launches
 launches   every launch of the device path on its own, in order: milliseconds; for convolutions also GMAC, TFLOP/s and the fraction of the
            157.3 TFLOP/s f32-MFMA pipe (the four heaviest are the ones DESIGN 5q quotes)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
ITEMS = {"head": 500, "launches": 500}   # seconds
PEAK_F32_MFMA = 157.3e12


def measure(sides, warm=5, runs=30):
    import torch
    out = {k: [] for k in sides}
    for i in range(warm + runs):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warm:
                out[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90))) for k, v in out.items()}


def record_launches(lib, fn):
    """run fn() once with the four library calls of the head wrapped: -> [(kind, args, kwargs, macs)] in launch order"""
    calls, saved = [], {}

    def wrap(name, macs):
        orig = getattr(lib, name)
        saved[name] = orig

        def inner(*a, **kw):
            calls.append((name, a, kw, macs(*a, **kw)))
            return orig(*a, **kw)
        setattr(lib, name, inner)
    osz = lambda size, k, s, p, d: lib.conv_out_size(size[0], k, s, p, d) * lib.conv_out_size(size[1], k, s, p, d)
    wrap("conv2d_rows_act", lambda x, size, w, k, bias=None, stride=1, padding=0, dilation=1, *a, **kw:
         osz(size, k, stride, padding, dilation) * w.shape[0] * w.shape[1])
    wrap("conv_transpose2d_rows", lambda x, size, w, s, *a, **kw: size[0] * size[1] * w.shape[0] * w.shape[1])
    wrap("conv2d_rows_project", lambda x, size, w1, k, b1, w2, b2=None, stride=1, padding=0, dilation=1, **kw:
         osz(size, k, stride, padding, dilation) * (w1.shape[0] * w1.shape[1] + w1.shape[0]))
    wrap("resize_rows", lambda *a, **kw: 0)
    try:
        fn()
    finally:
        for name, orig in saved.items():
            setattr(lib, name, orig)
    return calls, saved


def run_item(item):
    import torch
    from diffreg_hip import lib
    from diffreg_hip.dpt2d3d import DeviceDPTHead
    from tests import dpt2d3d_ref as R
    torch.set_grad_enabled(False)
    P = R.PRODUCTION
    ph, pw = P["grid"]
    m = R.DPTHead(P["in_channels"], P["features"], P["out_channels"]).to(DEV).eval()
    m.load_state_dict(R.draw_weights(m, 7, device=DEV))
    feats = R.make_inputs((ph, pw), 8, in_channels=P["in_channels"], device=DEV)
    head = DeviceDPTHead(m)
    calls, _ = record_launches(lib, lambda: head.forward(feats, ph, pw))
    gmac = sum(c[3] for c in calls) / 1e9
    if item == "head":
        a, b = head.forward(feats, ph, pw), m(feats, ph, pw)
        dev = R.rel_dev(a, b)
        assert dev < 1e-3, dev
        del a, b
        r = measure({"torch": lambda: m(feats, ph, pw), "device": lambda: head.forward(feats, ph, pw)})
        r["device"]["rel_dev_from_torch"] = dev
        r["gmac"], r["launches"] = gmac, len(calls)
        for side in ("torch", "device"):
            r[side]["tflops"] = 2e9 * gmac / (r[side]["median"] * 1e-3) / 1e12
        return r
    res = []
    for i, (name, a, kw, macs) in enumerate(calls):
        fn = getattr(lib, name)
        r = measure({"device": lambda: fn(*a, **kw)}, warm=3, runs=15)["device"]
        r.update(launch=i, kind=name, rows_in=int(a[0].shape[0]), cin=int(a[0].shape[1]), size=[int(v) for v in a[1]], gmac=macs / 1e9)
        if macs:
            r["cout"] = int(a[2].shape[0])
            r["tflops"] = 2.0 * macs / (r["median"] * 1e-3) / 1e12
            r["fraction_of_f32_mfma_pipe"] = 2.0 * macs / (r["median"] * 1e-3) / PEAK_F32_MFMA
        res.append(r)
    return res


def main():
    if "--item" in sys.argv:
        print("RESULT " + json.dumps(run_item(sys.argv[sys.argv.index("--item") + 1])))
        return 0
    res = {}
    for item, limit in ITEMS.items():
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--item", item], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print("%s: no result within %d s; stopping" % (item, limit))
            return 1
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("%s: exit status %d; stopping\n%s" % (item, p.returncode, p.stderr[-2000:]))
            return 1
        r = res[item] = json.loads(line[0][len("RESULT "):])
        if item == "head":
            print("head: %.1f GMAC in %d launches;  " % (r["gmac"], r["launches"]) +
                  "  ".join("%s %.3f [%.3f-%.3f] ms (%.1f TFLOP/s)" % (s, r[s]["median"], r[s]["p10"], r[s]["p90"], r[s]["tflops"]) for s in ("torch", "device")) +
                  ";  device / torch = %.2f" % (r["device"]["median"] / r["torch"]["median"]), flush=True)
        else:
            for c in r:
                tail = "" if not c["gmac"] else "  %6.2f GMAC  %5.1f TFLOP/s = %.3f of the f32-MFMA pipe" % (c["gmac"], c["tflops"], c["fraction_of_f32_mfma_pipe"])
                print("%2d %-22s %4d x %-4d %5d -> %-5s %8.3f [%.3f-%.3f] ms%s" % (c["launch"], c["kind"], c["size"][0], c["size"][1], c["cin"],
                                                                                  c.get("cout", ""), c["median"], c["p10"], c["p90"], tail), flush=True)
            print("sum of the launches' medians: %.3f ms" % sum(c["median"] for c in r))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
