"""Time the 2D-3D image backbone's inference forward on one GPU:

    python tools/image_backbone2d3d_time.py [--out FILE.json]

Geometry: one 480 x 640 gray image, 128 base channels, 128 output channels, DINO grid 34 x 45 x 512 (EXP/model.py:190-200, :358-361).  Method of
DESIGN 5f-5l: 5 warm-up runs, then 30 runs alternating the two sides, each between two device synchronisations; median [p10-p90] in milliseconds.
The baseline is the reference-shaped module (tests/image_backbone2d3d_ref.ImageBackbone: nothing is read from the reference) in plain
PyTorch float32 on the same GPU, under torch.no_grad().  Every item runs in a child process of its own under its own time limit; the first one
that fails ends the run.  Items:
 backbone   DeviceImageBackbone.forward (NCHW lists out, as the drop-in returns them) against the module's own forward; also forward_rows alone
 conv3x3    each distinct 3 x 3 launch of that forward on its own: milliseconds, TFLOP/s and the fraction of the 157.3 TFLOP/s f32-MFMA pipe, and
            torch's conv2d on the same NCHW problem"""
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
ITEMS = {"backbone": 400, "conv3x3": 400}   # seconds
PEAK_F32_MFMA = 157.3e12
# (stride, Cin, Cout, Hi, Wi): the 3 x 3 launches of the forward at 480 x 640 and 128 base channels, and how often each occurs
CONV3X3 = {"s1_128_128_240x320": (1, 128, 128, 240, 320, 4), "s2_128_256_240x320": (2, 128, 256, 240, 320, 2),
           "s1_256_256_120x160": (1, 256, 256, 120, 160, 3), "s2_256_512_120x160": (2, 256, 512, 120, 160, 2),
           "s1_512_512_60x80": (1, 512, 512, 60, 80, 3), "s1_512_512_120x160": (1, 512, 512, 120, 160, 1),
           "s1_512_256_120x160": (1, 512, 256, 120, 160, 1), "s1_256_256_240x320": (1, 256, 256, 240, 320, 1),
           "s1_256_128_240x320": (1, 256, 128, 240, 320, 1), "s1_128_128_480x640": (1, 128, 128, 480, 640, 2)}


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


def run_item(item):
    import torch
    import torch.nn.functional as TF
    from diffreg_hip import lib
    from diffreg_hip.image_backbone2d3d import DeviceImageBackbone
    from tests import image_backbone2d3d_ref as R
    torch.set_grad_enabled(False)
    if item == "backbone":
        case = R.PRODUCTION
        m = R.ImageBackbone(1, case["out"], case["base"]).to(DEV).eval()
        m.load_state_dict(R.make_weights(m, case["seed"], device=DEV))
        x, dino = R.make_inputs(case, device=DEV)
        ib = DeviceImageBackbone(m)
        a, b = ib.forward(x, dino), m(x, dino)
        dev = [R.rel_dev(p, q) for p, q in zip(a, b)]
        assert max(dev) < 1e-4, dev
        del a, b
        r = measure({"torch": lambda: m(x, dino), "device": lambda: ib.forward(x, dino), "device_rows": lambda: ib.forward_rows(x, dino)})
        r["device"]["max_rel_dev_from_torch"] = max(dev)
        return r
    res = {}
    for name, (s, cin, cout, H, W, count) in CONV3X3.items():
        g = torch.Generator(device=DEV).manual_seed(5)
        x = torch.randn(1, cin, H, W, generator=g, device=DEV)
        w = torch.randn(cout, cin, 3, 3, generator=g, device=DEV) * (1.0 / (9 * cin)) ** 0.5
        b = torch.zeros(cout, device=DEV)
        xr, wp = x[0].permute(1, 2, 0).reshape(H * W, cin).contiguous(), lib.pack_conv_weight(w)
        Ho, Wo = lib.conv_out_size(H, 3, s, 1), lib.conv_out_size(W, 3, s, 1)
        out = torch.empty(Ho * Wo, cout, device=DEV)
        r = measure({"torch": lambda: TF.conv2d(x, w, b, stride=s, padding=1), "device": lambda: lib.conv2d_rows(xr, (H, W), wp, 3, b, s, 1, 1, out=out)})
        flop = 2.0 * Ho * Wo * cout * 9 * cin
        for side in r.values():
            side["tflops"] = flop / (side["median"] * 1e-3) / 1e12
            side["fraction_of_f32_mfma_pipe"] = flop / (side["median"] * 1e-3) / PEAK_F32_MFMA
        r["gflop"], r["launches_per_forward"] = flop / 1e9, count
        res[name] = r
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
        res[item] = json.loads(line[0][len("RESULT "):])
        fmt = lambda sides: "  ".join("%s %.3f [%.3f-%.3f] ms" % (s, r["median"], r["p10"], r["p90"]) for s, r in sides.items() if isinstance(r, dict))
        if item == "backbone":
            print("%-22s" % item, fmt(res[item]), flush=True)
        else:
            for name, r in res[item].items():
                print("%-22s" % name, fmt(r), " device %.1f TFLOP/s = %.3f of the f32-MFMA pipe (torch %.1f); %.1f GFLOP x %d per forward"
                      % (r["device"]["tflops"], r["device"]["fraction_of_f32_mfma_pipe"], r["torch"]["tflops"], r["gflop"], r["launches_per_forward"]),
                      flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
