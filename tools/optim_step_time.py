"""Time the closing leg of a training iteration -- gradient gate + optimizer update + zero_grad -- on one GPU, three ways.

    python tools/optim_step_time.py [--runs 30] [--warmup 3] [--out FILE.json]

Two parameter sets, by shape only (random values; the leg does not depend on them):
  3dmatch   every parameter of the Pipeline that bench.py::bench_train_step trains (44.9 M), SGD lr 0.015, momentum 0.93, weight decay 1e-6
            (3D/main.py:90-96)
  2d3d      the trainable modules of the 2D-3D model as tests/train2d3d_ref.HostTrain2D3D states them, Adam lr 1e-4, weight decay 1e-6
            (vision3d/utils/optimizer.py:134-141)
Arms, alternated inside every run, 30 runs after warm-up, device-synchronised host clock; median and p10 - p90:
  (a) reference   the reference's leg verbatim: the per-tensor isnan / isinf loop of validate_gradient (two host reads per tensor), then torch's
                  optimizer.step() and zero_grad()
  (b) torch_best  one torch._foreach_norm over all gradients, one host read of its isfinite sum, then SGD / Adam(fused=True).step(), zero_grad()
  (c) device      diffreg_hip.optim.accelerate(gate=True, zero_grads=True): step() and zero_grad(), no host read
Before every timed window each arm's gradients are refilled from one source (the stand-in for backward; not timed).  For (c) the bytes the
kernels must move (gate 4 B + update 20 B (SGD with momentum) or 28 B (Adam) + 4 B of zeroed gradient per parameter) over the median give the
achieved rate, reported against the 6.29 TB/s float4 copy rate of DESIGN section 3.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

COPY_RATE = 6.29e12


def shapes_3dmatch():
    from bench import _attr
    from diffreg_hip import synth
    from models.pipeline import Pipeline
    v = synth.VARIANTS["3dmatch"]
    matching = dict(feature_dim=v["C"], confidence_threshold=0.2, entangled=False, dsmax_temperature=0.1, match_type="sinkhorn", skh_init_bin_score=1.0,
                    skh_iters=3, skh_prefilter=False)
    cfg = _attr(dict(dataset="3dmatch", coarse_matching=matching, SAMPLE_STEP=20,
                     kpfcn_config=dict(synth.KPFCN_CFG, architecture=list(synth.KPFCN_ARCH), KP_influence="linear", aggregation_mode="sum", deformable=False,
                                       use_batch_norm=True, fine_feature_dim=264, coarse_level=-2),
                     coarse_transformer=dict(feature_dim=v["C"], n_head=v["H"], layer_types=["self", "cross", "positioning", "self", "cross"],
                                             positioning_type="procrustes", pe_type="rotary", vol_bnds=[list(v["origin"]), [1.093, 0.78, 2.92]],
                                             voxel_size=v["voxel"], feature_matching=dict(matching), entangled=False,
                                             procrustes=dict(max_condition_num=200.0, sample_rate=1.0))))
    return [tuple(p.shape) for p in Pipeline(cfg).parameters() if p.requires_grad]


def shapes_2d3d():
    from tests import train2d3d_ref as R
    return [tuple(p.shape) for p in R.HostTrain2D3D().parameters() if p.requires_grad]


def reference_gate(params):
    """validate_gradient, 3D/lib/utils.py:96-106"""
    for p in params:
        if p.grad is not None:
            if torch.any(torch.isnan(p.grad)):
                return False
            if torch.any(torch.isinf(p.grad)):
                return False
    return True


def foreach_gate(params):
    norms = torch._foreach_norm([p.grad for p in params if p.grad is not None])
    return bool(torch.isfinite(torch.stack(norms).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_step_time: needs a GPU (a CPU run says nothing about the device)")
    from diffreg_hip import optim as dopt
    dev = "cuda:0"
    res = {"tool": "optim_step_time", "runs": a.runs, "copy_rate_Bps": COPY_RATE}
    sets = (("3dmatch", shapes_3dmatch(), "SGD", dict(lr=0.015, momentum=0.93, weight_decay=1e-6), 28),
            ("2d3d", shapes_2d3d(), "Adam", dict(lr=1e-4, weight_decay=1e-6), 36))
    for name, shapes, kind, opts, bytes_per_param in sets:
        gen = torch.Generator(device=dev).manual_seed(5)
        source = [0.01 * torch.randn(s, device=dev, generator=gen) for s in shapes]
        init = [torch.randn(s, device=dev, generator=gen) for s in shapes]
        n_param = sum(t.numel() for t in init)
        cls = getattr(torch.optim, kind)
        arms = {}
        for arm, kw in (("reference", {}), ("torch_best", {"fused": True}), ("device", {})):
            params = [t.clone() for t in init]
            arms[arm] = (params, cls(params, **opts, **kw))
        dopt.accelerate(arms["device"][1], gate=True, zero_grads=True)

        def leg(arm):
            params, opt = arms[arm]
            if arm == "reference":
                if reference_gate(params):
                    opt.step()
                opt.zero_grad()
            elif arm == "torch_best":
                if foreach_gate(params):
                    opt.step()
                opt.zero_grad()
            else:
                opt.step()
                opt.zero_grad()

        def refill(arm):
            for p, g in zip(arms[arm][0], source):
                if p.grad is None:
                    p.grad = g.clone()
                else:
                    p.grad.copy_(g)

        t = {arm: [] for arm in arms}
        for it in range(a.warmup + a.runs):
            for arm in arms:
                refill(arm)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg(arm)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    t[arm].append((time.perf_counter() - t0) * 1e3)
        entry = {"optimizer": kind, "options": opts, "tensors": len(shapes), "parameters": n_param,
                 "device_steps_taken": dopt.steps_taken(arms["device"][1]), "device_steps_skipped": dopt.skipped_steps(arms["device"][1])}
        # the three arms started from the same values and saw the same gradients: how far apart they ended
        dev_p = arms["device"][0]
        for arm in ("reference", "torch_best"):
            entry["max_abs_diff_device_vs_" + arm] = max(float((p - q).abs().max()) for p, q in zip(dev_p, arms[arm][0]) if p.numel())
        for arm, v in t.items():
            v = np.array(v)
            entry[arm + "_ms"] = {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))}
        need = bytes_per_param * n_param
        rate = need / (entry["device_ms"]["median"] * 1e-3)
        entry["device_bytes_needed"] = need
        entry["device_achieved_Bps"] = rate
        entry["device_share_of_copy_rate"] = rate / COPY_RATE
        res[name] = entry
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
