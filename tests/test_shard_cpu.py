"""N > 1 path on CPU: pair sharding + metric gather with world_size 2 over gloo; package overlay."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.conftest import ROOT


def _worker(rank, world, port, n_pairs, q):
    sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
    from diffreg_hip import shard
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    mine = shard.shard_pairs(n_pairs, rank, world)
    # stand-in per-pair metrics: IR_i = i/100, FMR_i = [IR_i > 0.05]
    ir = [i / 100.0 for i in mine]
    sums = shard.gather_metrics([sum(ir), sum(1.0 for v in ir if v > 0.05), float(len(mine))])
    tmax = shard.max_over_ranks(1.0 + rank)
    q.put((rank, mine, sums.tolist(), tmax))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_shard_and_gather():
    world, n_pairs = 2, 13
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 1000)
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_pairs, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    owned = sorted(i for _, mine, _, _ in res for i in mine)
    assert owned == list(range(n_pairs))                               # every pair exactly once
    assert abs(len(res[0][1]) - len(res[1][1])) <= 1
    want = [sum(i / 100.0 for i in range(n_pairs)), float(sum(1 for i in range(n_pairs) if i / 100.0 > 0.05)), float(n_pairs)]
    for _, _, sums, tmax in res:
        assert sums == pytest.approx(want) and tmax == 2.0


def _run_bench_stub(nproc, extra, gpus=None, expect_fail=False):
    """bench.py's own multi-rank control path (torchrun environment, barrier, max time over ranks, metric-vector all_reduce: --full)
    under gloo with the CPU stand-in engine (--cpu-stub)"""
    import json
    import subprocess
    port = 29600 + (os.getpid() % 300)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(nproc if gpus is None else gpus), "--steps", "3",
           "--warmup", "1", "--cpu-stub", "--full"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    if expect_fail:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                       # rank 0 prints ONE line
    return json.loads(lines[0])


def test_bench_rank_path_two_ranks_weak_scaling():
    d = _run_bench_stub(2, ["--pairs", "6"])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "weak" and d["data"].startswith("cpu-stub")
    mg = d["metric_gather"]
    ids = list(range(12))                                            # rank r owns pairs 6 r .. 6 r + 5
    assert mg["n_pairs"] == 12 and mg["per_rank_pairs"] == [6, 6] and mg["backend"] == "gloo"
    assert mg["sum_inlier_ratio"] == pytest.approx(sum((i % 10) / 10.0 for i in ids))
    assert mg["sum_fmr"] == pytest.approx(sum(1.0 for i in ids if (i % 10) / 10.0 > 0.05))
    assert mg["sum_registration_recall"] == pytest.approx(sum(1.0 for i in ids if i % 3 == 0))
    # value = pairs of ALL ranks x steps / max-over-ranks time
    assert d["value"] == pytest.approx(12 * 3 / (d["ms_per_step"] * 3e-3), rel=1e-6)
    assert len(mg["per_rank_pairs_per_s"]) == 2 and all(v > 0 for v in mg["per_rank_pairs_per_s"])


def test_bench_rank_path_ragged_shard():
    """13 pairs round-robin over 2 ranks (7 + 6: BASELINE configs[3]-style sharding of a fixed set): the gather still counts
    every pair once, and the slower rank (more pairs) sets the time"""
    d = _run_bench_stub(2, ["--total-pairs", "13"])
    mg = d["metric_gather"]
    assert mg["n_pairs"] == 13 and sorted(mg["per_rank_pairs"]) == [6, 7]
    assert mg["sum_inlier_ratio"] == pytest.approx(sum((i % 10) / 10.0 for i in range(13)))
    assert mg["sum_registration_recall"] == pytest.approx(sum(1.0 for i in range(13) if i % 3 == 0))
    assert d["value"] == pytest.approx(13 * 3 / (d["ms_per_step"] * 3e-3), rel=1e-6)


def test_bench_cfg4_sharding_and_gpus_world_size_mismatch():
    """BASELINE configs[3]: 64 pairs sharded over the ranks.  Under world size 2 every pair is owned exactly once (32 + 32), and a
    `--gpus 8` that does not match the launched world size is refused instead of reported as an 8-GPU line."""
    d = _run_bench_stub(2, ["--total-pairs", "64"])
    mg = d["metric_gather"]
    assert d["n_gpus"] == 2 and mg["n_pairs"] == 64 and sum(mg["per_rank_pairs"]) == 64 and mg["per_rank_pairs"] == [32, 32]
    assert mg["sum_inlier_ratio"] == pytest.approx(sum((i % 10) / 10.0 for i in range(64)))
    r = _run_bench_stub(2, ["--total-pairs", "64"], gpus=8, expect_fail=True)
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr and not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_metric_vector_of_evaluate_pairs_shaped_data():
    """shard.metric_vector / reduce_metrics on the dict layout diffreg_hip.metrics.evaluate_pairs returns (ir, fmr, rr_ok [P])"""
    from diffreg_hip import shard
    ev = dict(ir=torch.tensor([0.5, 0.02, 0.3]), fmr=torch.tensor([1.0, 0.0, 1.0]), rr_ok=torch.tensor([1, 0, 0], dtype=torch.int32))
    v = shard.metric_vector(ev["ir"], ev["fmr"], ev["rr_ok"], 2.5)
    assert v.dtype == torch.float64 and v.tolist() == pytest.approx([0.82, 2.0, 1.0, 3.0, 2.5])
    g = shard.reduce_metrics(v)
    assert g["mean_inlier_ratio"] == pytest.approx(0.82 / 3) and g["fmr"] == pytest.approx(2 / 3) and g["n_pairs"] == 3


def test_single_process_gather_is_identity():
    from diffreg_hip import shard
    assert shard.shard_pairs(5, 0, 1) == [0, 1, 2, 3, 4]
    assert shard.gather_metrics([1.0, 2.0]).tolist() == [1.0, 2.0]


def _stand_in_reference_tree(root):
    """a checkout with the reference's package layout (3D/models, 3D/models/transformer, 3D/kernels): the modules the overlay shadows
    are decoys that fail on import, the ones it leaves to the checkout are one-liners that record where they were found"""
    files = {"models/__init__.py": "", "models/transformer/__init__.py": "", "kernels/__init__.py": "",
             "kernels/kernel_points.py": "HOME = 'tree'\n",
             "models/blocks.py": "from kernels.kernel_points import HOME\n",
             "models/transformer/geoattention.py": "HOME = 'tree'\n",
             "models/transformer/geotransformer.py": "from models.transformer.geoattention import HOME\n"}
    for name in ("pipeline", "backbone", "matching", "procrustes", "transformero", "position_encoding", "loss"):
        files["models/%s.py" % name] = "raise ImportError('the checkout shadowed the overlay: models.%s')\n" % name
    for rel, text in files.items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    return str(root)


def test_models_overlay_resolves_the_rest_in_reference_tree(tmp_path):
    """our models.* shadow the hot-path modules (and the backbone, row f1); everything else (models.blocks, models.loss,
    models.transformer.geotransformer, ...) still comes from the reference checkout -- here a stand-in with its package layout."""
    import subprocess
    tree = _stand_in_reference_tree(tmp_path / "Diff-Reg-3dmatch")
    code = ("import sys; sys.path.insert(0,%r); sys.path.insert(0,%r);"
            "import models.pipeline as p, models.backbone as b, models.blocks as k, models.transformer.geotransformer as g;"
            "from models.transformer import RepositioningTransformer as R;"
            "assert p.__file__.startswith(%r) and b.__file__.startswith(%r) and k.__file__.startswith(%r) and g.__file__.startswith(%r) "
            "and k.HOME == g.HOME == 'tree' and R.__module__=='models.transformero';"
            "print('ok')") % (tree, os.path.join(ROOT, "diff-reg_amd"), ROOT, ROOT, tree, tree)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def test_backbone_overlay_state_dict_matches_reference():
    """models/backbone.py exposes exactly the reference KPFCN's parameter names and shapes, so the
    `backbone.*` part of a Diff-Reg checkpoint loads unchanged (names / shapes recorded from the reference module by
    oracle/make_golden_kpfcn.py)."""
    import importlib.util
    import numpy as np
    from diffreg_hip import synth
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("dr_models_backbone", os.path.join(here, "..", "diff-reg_amd", "models", "backbone.py"))
    mb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mb)
    cfg = dict(synth.KPFCN_CFG, architecture=list(synth.KPFCN_ARCH), KP_influence="linear", aggregation_mode="sum", deformable=False,
               use_batch_norm=True, fine_feature_dim=264)
    mine = {k: tuple(v.shape) for k, v in mb.KPFCN(cfg).state_dict().items()}
    g = np.load(os.path.join(here, "golden", "kpfcn_coarse.npz"))
    ref = {str(k): tuple(int(v) for v in str(s).split(";") if v) for k, s in zip(g["sd_keys"], g["sd_shapes"])}
    assert mine == ref
