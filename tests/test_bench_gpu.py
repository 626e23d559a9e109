"""bench.py's plain run on the device: the line carries the contract fields and nothing of --full, and --dump-outputs writes what the
last timed step computed -- the same numbers an eager run of the same batches returns.  Needs a GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--pairs", "8", "--streams", "2",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["value"] == pytest.approx(8 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    assert d["unit"] == "pairs/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert not any(k in d for k in ("metric_gather", "roofline", "sinkhorn_roofline", "single_pair", "other_configs", "cpu_baseline"))
    files = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}
    assert set(files) == {"R_final", "t_final", "match_count", "match_pred", "sample_pairs", "conf_matrix_pred", "x_final"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir)) <= 64 << 20
    assert files["sample_pairs"].tolist() == list(range(8)) and files["conf_matrix_pred"].shape == (8, 256, 256)
    # the same two batches run eagerly, in-process: the dump holds what the timed path returned
    sys.path.insert(0, ROOT)
    import bench
    _, eng = bench.make_engine("3dmatch", 20, 200.0, "cuda:0")
    for g, ids in enumerate(([0, 1, 2, 3], [4, 5, 6, 7])):
        _, inp = bench.make_inputs("3dmatch", 4, 256, 256, 0, "cuda:0", seeds=[5000 + i for i in ids])
        o = eng.run(inp["f_s"], inp["f_t"], inp["p_s"], inp["p_t"], inp["x_T"], _slot=g)
        torch.cuda.synchronize()
        assert np.abs(o["conf_matrix_pred"].cpu().numpy() - files["conf_matrix_pred"][ids]).max() < 1e-6
        assert np.abs(o["R_final"].cpu().numpy() - files["R_final"][ids]).max() < 1e-5
        cnt = o["match_count"].cpu().numpy()
        assert np.array_equal(cnt, files["match_count"][ids])
        for k, i in enumerate(ids):
            assert np.array_equal(o["matches_padded"][k, :cnt[k]].cpu().numpy(), files["match_pred"][i, :cnt[k]])
            assert (files["match_pred"][i, cnt[k]:] == -1).all()
