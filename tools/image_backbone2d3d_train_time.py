"""Time the 2D-3D image backbone's forward + backward on one GPU:

    python tools/image_backbone2d3d_train_time.py [--out FILE.json]

Geometry: tests/image_backbone2d3d_ref.PRODUCTION -- one 480 x 640 gray image, 128 base channels, 128 output channels, DINO grid 34 x 45 x 512.
One run = zero the gradients, forward with gradients enabled, loss = the sum of the four outputs, backward; between two device synchronisations.
5 warm-up runs, then 30 runs; median [p10-p90] in milliseconds.  The baseline is the same module (tests/image_backbone2d3d_ref.ImageBackbone:
nothing is read from the reference) in plain PyTorch float32 on the same GPU.  Every item runs in a child process of its own under its own
time limit -- the two sides of the whole-backbone comparison never share an allocator or a kernel cache; the first item that fails ends the run.
 step_torch / step_device   the whole forward + backward, the module's own code / bound with grad=True
 conv3x3                    each distinct 3 x 3 launch of the backward on its own, data gradient and weight gradient (with grad_bias):
                            milliseconds, TFLOP/s and the fraction of the 157.3 TFLOP/s f32-MFMA pipe"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from image_backbone2d3d_time import CONV3X3, DEV, PEAK_F32_MFMA, measure  # noqa: E402

ITEMS = {"step_torch": 400, "step_device": 400, "conv3x3": 400}   # seconds


def run_item(item):
    import torch
    from diffreg_hip import lib
    from diffreg_hip.image_backbone2d3d import bind
    from tests import image_backbone2d3d_ref as R
    if item in ("step_torch", "step_device"):
        case = R.PRODUCTION
        m = R.ImageBackbone(1, case["out"], case["base"]).to(DEV).train()
        m.load_state_dict(R.make_weights(m, case["seed"], device=DEV))
        x, dino = R.make_inputs(case, device=DEV)
        if item == "step_device":
            bind(m, grad=True)

        def step():
            m.zero_grad(set_to_none=True)
            sum(o.sum() for o in m(x, dino)).backward()
        r = measure({"step": step})["step"]
        r["grad_abs_sum"] = float(sum(p.grad.double().abs().sum() for p in m.parameters()))
        return r
    torch.set_grad_enabled(False)
    res = {}
    for name, (s, cin, cout, H, W, count) in CONV3X3.items():
        g = torch.Generator(device=DEV).manual_seed(5)
        Ho, Wo = lib.conv_out_size(H, 3, s, 1), lib.conv_out_size(W, 3, s, 1)
        x = torch.randn(H * W, cin, generator=g, device=DEV)
        go = torch.randn(Ho * Wo, cout, generator=g, device=DEV)
        wt = lib.pack_conv_weight_t(torch.randn(cout, cin, 3, 3, generator=g, device=DEV) * (1.0 / (9 * cin)) ** 0.5)
        gx = torch.empty(H * W, cin, device=DEV)
        r = measure({"dgrad": lambda: lib.conv2d_rows_backward_data(go, (H, W), wt, 3, s, 1, 1, out=gx),
                     "wgrad": lambda: lib.conv2d_rows_backward_weight(x, (H, W), go, 3, s, 1, 1, packed=True)})
        flop = 2.0 * Ho * Wo * cout * 9 * cin                       # the useful multiply-adds: the forward's, for either gradient
        for side in r.values():
            side["tflops"] = flop / (side["median"] * 1e-3) / 1e12
            side["fraction_of_f32_mfma_pipe"] = flop / (side["median"] * 1e-3) / PEAK_F32_MFMA
        r["gflop"], r["launches_per_backward"], r["slabs"] = flop / 1e9, count, lib.conv_wgrad_slabs(Ho * Wo)[0]
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
        res[item] = r = json.loads(line[0][len("RESULT "):])
        if item != "conv3x3":
            print("%-22s %.3f [%.3f-%.3f] ms" % (item, r["median"], r["p10"], r["p90"]), flush=True)
        else:
            for name, c in r.items():
                print("%-22s" % name, "  ".join("%s %.3f [%.3f-%.3f] ms = %.1f TFLOP/s = %.3f of the f32-MFMA pipe"
                                                % (k, c[k]["median"], c[k]["p10"], c[k]["p90"], c[k]["tflops"], c[k]["fraction_of_f32_mfma_pipe"])
                                                for k in ("dgrad", "wgrad")), "; %.1f GFLOP x %d, %d slabs" % (c["gflop"], c["launches_per_backward"], c["slabs"]),
                      flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
