"""bench.py's plain run, --full and --dump-outputs on the GPU, at reduced sizes: a plain run times exactly --steps steps and
carries none of the extras; --dump-outputs writes what the last timed step computed, and the same arguments give the same
inputs, so a plain and a --full run dump the same MSM total -- the one the --full run's CPU baseline checks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(*args, timeout=600):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MLHIP_BENCH_REHEARSAL"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args), env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_and_full_runs_dump_the_same_msm(tmp_path):
    plain, full = tmp_path / "plain", tmp_path / "full"
    d = _bench("--log-n", "14", "--steps", "3", "--warmup", "1", "--dump-outputs", str(plain))
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "scalar-muls/s" and d["dtype"] == "u32"
    assert d["cpu_baseline"] is None and "pcie_inclusive" not in d["extra"] and "pairings_per_s_per_gpu" not in d["extra"]
    assert sorted(f for f in os.listdir(plain) if f.endswith(".npy")) == ["msm_g1.npy"]
    f = _bench("--log-n", "14", "--steps", "2", "--warmup", "1", "--full", "--dump-outputs", str(full))
    assert f["cpu_baseline"]["matches_gpu_result"] and f["extra"]["pcie_inclusive"]["match_resident_result"]
    a, b = np.load(plain / "msm_g1.npy"), np.load(full / "msm_g1.npy")
    assert a.dtype == np.float64 and a.shape == (2, 48) and a.any()
    assert np.array_equal(a, b)


def test_pairing_batch_dump(tmp_path):
    d = _bench("--config", "3", "--log-n", "10", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["unit"] == "pairings/s" and d["cpu_baseline"] is None
    gt, idx = np.load(tmp_path / "pairing_gt.npy"), np.load(tmp_path / "pairing_gt_index.npy")
    assert gt.shape == (1024, 12, 48) and np.array_equal(idx, np.arange(1024)) and gt.any()
    assert ((gt >= 0) & (gt < 256) & (gt == np.round(gt))).all()
