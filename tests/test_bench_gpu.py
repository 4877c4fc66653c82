"""GPU: bench.py's own contract.  A plain run prints the headline line and nothing it does not need; --full adds
the roofline and the self-check of the timed outputs; --dump-outputs writes the maps of the last timed step, which
must be the reference's maps of the crops they were computed from."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H

GOLD = ["urban1_robotics", "urban2_kitti", "urban3_kitti", "urban4_kitti"]   # pair i of the batch is crop i % 4


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "bench.py"), "--gpus", "1", "--batch", "64",
                        "--spinup", "0"] + list(args), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_last_step(tmp_path):
    d = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "pairs/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["ranks"][0]["pairs"] == 3 * 64
    for k in ("roofline", "golden_check", "cpu_baseline", "matcher", "throughput_host_buffers"):
        assert k not in d, k
    assert sorted(os.listdir(tmp_path)) == ["D1.npy", "D2.npy", "pair_index.npy"]
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 * 10 ** 6
    idx = np.load(tmp_path / "pair_index.npy")
    D1, D2 = np.load(tmp_path / "D1.npy"), np.load(tmp_path / "D2.npy")
    assert idx.dtype == np.float64 and D1.dtype == np.float32 and D2.dtype == np.float32
    assert len(idx) == 8 and len(set(idx.tolist())) == 8 and idx.min() >= 0 and idx.max() < 64
    assert D1.shape == D2.shape == (8, 375, 1242)
    for k, i in enumerate(idx.astype(int)):
        z = np.load(os.path.join(H.GOLDEN, GOLD[i % 4] + ".npz"))
        assert np.array_equal(D1[k].ravel(), z["d1"]), (k, i)
        assert np.array_equal(D2[k].ravel(), z["d2"]), (k, i)


@pytest.mark.gpu
def test_bench_full_run_checks_itself():
    d = _bench("--steps", "2", "--warmup", "1", "--full", "--no-extras", "--no-cpu-baseline")
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["roofline"] and d["roofline"]["kernel"] and d["roofline"]["achieved"] > 0
    assert d["outputs_match_golden"] is True and d["golden_check"]["pairs_checked"] == 8
